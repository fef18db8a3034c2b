// zenc_fse_main.cpp -- writes one zstd frame from literals and sequence lists as the device
// encoder does in each of its three modes (0: raw literals, 1: OKV_F_ZSTD_HUFFMAN, 2: with
// OKV_F_ZSTD_HUF_FSE), using only objectkv_amd/csrc/okv_zstd_enc.hpp (the statements the
// device encoder runs) and a sequential bit writer.
// tests/test_zstd_fse_host.py builds it with AddressSanitizer and UBSan, runs it as a plain
// program and inflates the frames with libzstd.
//
//   zenc_fse_main <cases.bin> <frame.out>
// cases.bin (little endian): u64 content size, u32 checksum, u32 nblocks, u32 mode, then per
//   block  u32 nlit, nlit bytes, u32 nseq, nseq x (u32 ll, u32 ml, u32 off).
// A block is one unit: its source bytes are the literals with the matches copied in.  One line
// per block goes to stdout: tests/zenc_huf_main.cpp's, then
//   desc <0 direct | 1 FSE: the description the Huffman section has or would have>
//   dbytes <its bytes with the header byte, 0: none>  dfse <the FSE one's, 0: none>
//   ddir <the direct one's, 0: none>  alog <accuracy log of the FSE one, 0: none>
//
//   zenc_fse_main --lens <hists.bin> <lens.out>
// hists.bin: histograms of 256 u32; lens.out per histogram: u32 longest length and 256 u32
//   lengths over all byte values, then u32 longest and 129 u32 lengths of huf_lengths.
//
//   zenc_fse_main --desc <weights.bin> <sizes.out>
// weights.bin: lists of u32 n, n weight bytes; sizes.out per list u32 bytes of the FSE
//   description without its header byte (0: none, or more than 127) and u32 accuracy log.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "okv_zstd_enc.hpp"

namespace ze = okv::zenc;

struct Seq {
  uint32_t ll, ml, off;
};

static std::vector<uint8_t> in;
static size_t at = 0;

static uint64_t rd(unsigned n) {
  if (at + n > in.size()) {
    std::fprintf(stderr, "short case file\n");
    std::exit(2);
  }
  uint64_t v = 0;
  for (unsigned i = 0; i < n; ++i) v |= uint64_t(in[at + i]) << (8 * i);
  at += n;
  return v;
}

struct BitWriter {  // low bits first
  std::vector<uint8_t>& out;
  size_t base;
  uint64_t nbits = 0;
  BitWriter(std::vector<uint8_t>& o) : out(o), base(o.size()) {}
  void add(uint64_t v, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i, ++nbits) {
      if ((nbits & 7) == 0) out.push_back(0);
      if ((v >> i) & 1) out[base + (nbits >> 3)] |= uint8_t(1u << (nbits & 7));
    }
  }
  void add(const ze::SeqBits& b) {
    add(b.lo, b.nb < 64 ? b.nb : 64);
    if (b.nb > 64) add(b.hi, b.nb - 64);
  }
};

static void put(std::vector<uint8_t>& out, const uint8_t* p, size_t n) {
  out.insert(out.end(), p, p + n);
}
static void put32(std::vector<uint8_t>& out, uint32_t v) {
  for (int k = 0; k < 4; ++k) out.push_back(uint8_t(v >> (8 * k)));
}

static bool read_file(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  for (int c; (c = std::fgetc(f)) != EOF;) in.push_back(uint8_t(c));
  std::fclose(f);
  return true;
}

static bool write_file(const char* path, const std::vector<uint8_t>& out) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  std::fwrite(out.data(), 1, out.size(), f);
  std::fclose(f);
  return true;
}

static int lens_mode(const char* src, const char* dst) {
  if (!read_file(src) || in.size() % 1024) return 2;
  std::vector<uint8_t> out;
  std::vector<uint32_t> work(ze::kHufAllWork);
  static_assert(ze::kHufAllWork >= ze::kHufWork, "one work space for both");
  for (; at < in.size();) {
    uint32_t hist[256], len[ze::kHufAllSyms];
    for (uint32_t& h : hist) h = uint32_t(rd(4));
    std::memset(len, 0, sizeof len);
    put32(out, ze::huf_lengths_all(hist, len, work.data()));
    for (uint32_t s = 0; s < ze::kHufAllSyms; ++s) put32(out, len[s]);
    std::memset(len, 0, sizeof len);
    put32(out, ze::huf_lengths(hist, len, work.data()));
    for (uint32_t s = 0; s < ze::kHufSyms; ++s) put32(out, len[s]);
  }
  return write_file(dst, out) ? 0 : 2;
}

// The FSE description of the n weights in w.w: bytes without the header byte (0: none).
static uint32_t describe(ze::WtWork& w, uint32_t n, uint32_t& alog) {
  alog = 0;
  const uint32_t nc = ze::wt_prepare(w, n);
  if (!nc) return 0;
  ze::wt_chain(w, n, 0);
  ze::wt_chain(w, n, 1);
  alog = w.ct.log;
  return ze::wt_pack(w, n, nc);
}

static int desc_mode(const char* src, const char* dst) {
  if (!read_file(src)) return 2;
  std::vector<uint8_t> out;
  for (; at < in.size();) {
    const uint32_t n = uint32_t(rd(4));
    ze::WtWork w;
    std::memset(&w, 0, sizeof w);
    if (n > 255) return 2;
    for (uint32_t i = 0; i < n; ++i)
      if ((w.w[i] = uint8_t(rd(1))) >= ze::kWtSyms) return 2;
    uint32_t alog;
    put32(out, describe(w, n, alog));
    put32(out, alog);
  }
  return write_file(dst, out) ? 0 : 2;
}

// The Huffman literals section of `lits` in `mode` (1, 2), or nothing when there is no tree
// description for them.  The caller compares sizes.
struct HufInfo {
  uint32_t bits = 0, last = 0, streams = 0;
  uint32_t desc = 0, dbytes = 0, dfse = 0, ddir = 0, alog = 0;
};
static HufInfo huf_section(uint32_t mode, const uint8_t* lits, uint32_t nlit,
                           std::vector<uint8_t>& sec) {
  HufInfo hi;
  uint32_t hist[256] = {0};
  for (uint32_t i = 0; i < nlit; ++i) hist[lits[i]] += 1;
  std::vector<uint32_t> work(ze::kHufAllWork);
  uint32_t code[ze::kHufAllSyms] = {0};
  ze::WtWork w;
  std::memset(&w, 0, sizeof w);
  uint32_t fse_bytes = 0;
  if (mode == 2) {
    hi.bits = ze::huf_lengths_all(hist, code, work.data());
    if (!hi.bits) return hi;
    hi.last = ze::huf_codes_all(code, hi.bits, code, work.data());
    for (uint32_t s = 0; s < hi.last; ++s) w.w[s] = uint8_t(ze::huf_weight(code[s] & 15u, hi.bits));
    fse_bytes = describe(w, hi.last, hi.alog);
    if (!fse_bytes) hi.alog = 0;
  } else {
    hi.bits = ze::huf_lengths(hist, code, work.data());
    if (!hi.bits) return hi;
    hi.last = ze::huf_codes(code, hi.bits, code, work.data());
  }
  bool fse = false;
  hi.dbytes = ze::huf_desc_size(hi.last, fse_bytes, fse);
  hi.desc = fse ? 1 : 0;
  hi.dfse = fse_bytes ? 1 + fse_bytes : 0;
  hi.ddir = hi.last <= ze::kHufMaxSym ? ze::huf_tree_size(hi.last) : 0;
  if (!hi.dbytes) {  // a value above 128 and no FSE description: as if not eligible
    hi.bits = 0;
    return hi;
  }
  hi.streams = ze::huf_streams(nlit);
  std::vector<uint8_t> body;
  if (fse) {
    body.push_back(uint8_t(fse_bytes));
    put(body, w.out, fse_bytes);
  } else {
    for (uint32_t k = 0; k < ze::huf_tree_size(hi.last); ++k)
      body.push_back(ze::huf_tree_byte(code, hi.bits, hi.last, k));
  }
  if (body.size() != hi.dbytes) std::exit(3);
  const size_t jump = body.size();
  if (hi.streams == 4) body.resize(jump + 6);
  uint32_t first = 0, total = 0;
  for (uint32_t s = 0; s < hi.streams; ++s) {
    const uint32_t cnt = ze::huf_stream_len(nlit, s);
    const size_t start = body.size();
    BitWriter bw(body);
    for (uint32_t i = first + cnt; i-- > first;) bw.add(code[lits[i]] >> 4, code[lits[i]] & 15u);
    const uint32_t bytes = ze::huf_stream_bytes(uint32_t(bw.nbits));
    bw.add(1, 1);
    if (body.size() - start != bytes) std::exit(3);
    if (hi.streams == 4 && s < 3) {
      if (bytes > 0xFFFF) std::exit(3);
      body[jump + 2 * s] = uint8_t(bytes), body[jump + 2 * s + 1] = uint8_t(bytes >> 8);
    }
    total += bytes;
    first += cnt;
  }
  if (first != nlit) std::exit(3);
  uint8_t hb[8];
  put(sec, hb, ze::huf_header(hb, nlit, uint32_t(body.size())));
  put(sec, body.data(), body.size());
  if (sec.size() != ze::huf_section_size_d(nlit, hi.dbytes, total)) std::exit(3);
  if (!fse && sec.size() != ze::huf_section_size(nlit, hi.last, total)) std::exit(3);
  if ((sec.size() < ze::lit_header_size(nlit) + nlit) != ze::huf_wins_d(nlit, hi.dbytes, total))
    std::exit(3);
  return hi;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "--lens")) return lens_mode(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "--desc")) return desc_mode(argv[2], argv[3]);
  if (argc != 3 || !read_file(argv[1])) return 2;

  ze::CTable ct[3];
  for (uint32_t t = 0; t < 3; ++t) ze::build_ctable(ct[t], t);

  const uint64_t fcs = rd(8);
  const uint32_t checksum = uint32_t(rd(4));
  const uint32_t nblocks = uint32_t(rd(4));
  const uint32_t mode = uint32_t(rd(4));
  if (mode > 2) return 2;
  std::vector<uint8_t> out;
  uint8_t hb[16];
  put(out, hb, ze::frame_header(hb, fcs));
  for (uint32_t b = 0; b < nblocks; ++b) {
    const uint32_t nlit = uint32_t(rd(4));
    if (at + nlit > in.size()) return 2;
    const uint8_t* lits = in.data() + at;
    at += nlit;
    const uint32_t nseq = uint32_t(rd(4));
    std::vector<Seq> seqs(nseq);
    for (Seq& s : seqs) s.ll = uint32_t(rd(4)), s.ml = uint32_t(rd(4)), s.off = uint32_t(rd(4));
    // the unit's source bytes
    std::vector<uint8_t> unit;
    uint32_t lp = 0;
    for (const Seq& s : seqs) {
      if (lp + s.ll > nlit || s.off == 0 || s.off > unit.size() + s.ll) return 2;
      put(unit, lits + lp, s.ll);
      lp += s.ll;
      for (uint32_t j = 0; j < s.ml; ++j) unit.push_back(unit[unit.size() - s.off]);
    }
    put(unit, lits + lp, nlit - lp);
    const uint32_t n = uint32_t(unit.size());
    if (n > ze::kUnit) return 2;
    // the literals section
    std::vector<uint8_t> litsec, huf;
    HufInfo hi;
    if (mode) hi = huf_section(mode, lits, nlit, huf);
    const uint32_t raw_size = ze::lit_header_size(nlit) + nlit;
    const bool use_huf = hi.bits && huf.size() < raw_size;
    if (use_huf) {
      litsec = huf;
    } else {
      put(litsec, hb, ze::lit_header(hb, nlit));
      put(litsec, lits, nlit);
    }
    // the sequences section
    std::vector<uint8_t> seqsec;
    put(seqsec, hb, ze::nseq_header(hb, nseq));
    uint64_t bits = 0;
    if (nseq) {
      seqsec.push_back(0);  // Predefined_Mode for all three tables
      BitWriter bw(seqsec);
      uint32_t state[3];
      for (uint32_t t = 0; t < 3; ++t) {
        const Seq& s = seqs[nseq - 1];
        state[t] = ze::fse_init(ct[t], ze::seq_sym(t, s.ll, s.ml, s.off));
      }
      for (uint32_t k = nseq; k-- > 0;) {
        const Seq& s = seqs[k];
        const ze::SeqCode c = ze::seq_code(s.ll, s.ml, s.off);
        uint32_t nb[3] = {0, 0, 0}, sbits[3] = {0, 0, 0};
        if (k + 1 != nseq)
          for (uint32_t t = 0; t < 3; ++t)
            state[t] = ze::fse_step(ct[t], state[t], c.sym[t], nb[t], sbits[t]);
        bw.add(ze::seq_bits(c, nb, sbits));
      }
      bw.add(ze::close_bits(state));
      bits = bw.nbits;
    }
    const uint32_t csz = uint32_t(litsec.size() + seqsec.size());
    if (csz != ze::block_content_size(uint32_t(litsec.size()), nseq, bits)) return 3;
    if (!use_huf && nseq && csz != ze::compressed_size(nlit, nseq, bits)) return 3;
    const bool comp = csz < n;
    if (comp && !nseq && !use_huf) return 3;
    const bool last = b + 1 == nblocks;
    uint8_t bh[3];
    if (comp) {
      ze::block_header(bh, last, ze::kBlockCompressed, csz);
      put(out, bh, 3);
      put(out, litsec.data(), litsec.size());
      put(out, seqsec.data(), seqsec.size());
    } else {
      ze::block_header(bh, last, ze::kBlockRaw, n);
      put(out, bh, 3);
      put(out, unit.data(), n);
    }
    const uint32_t hs = ze::huf_header_size(nlit);
    const bool hufout = comp && use_huf;
    std::printf("block %u n %u nlit %u nseq %u lit %u streams %u sf %u huf %zu raw %u bits %u "
                "last %u csz %u desc %u dbytes %u dfse %u ddir %u alog %u\n",
                comp ? ze::kBlockCompressed : ze::kBlockRaw, n, nlit, nseq,
                hufout ? 2u : 0u, hufout ? hi.streams : 0u,
                hufout ? (hs == 3 ? 0u : hs == 4 ? 2u : 3u) : 0u, huf.size(), raw_size, hi.bits,
                hi.last, csz, hi.desc, hi.dbytes, hi.dfse, hi.ddir, hi.alog);
  }
  for (int i = 0; i < 4; ++i) out.push_back(uint8_t(checksum >> (8 * i)));
  if (!write_file(argv[2], out)) return 2;
  std::printf("frame of %zu bytes written\n", out.size());
  return 0;
}
