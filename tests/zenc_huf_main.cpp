// zenc_huf_main.cpp -- writes one zstd frame from literals and sequence lists as the device
// encoder does under OKV_F_ZSTD_HUFFMAN, using only objectkv_amd/csrc/okv_zstd_enc.hpp (the
// statements the device encoder runs) and a sequential bit writer: per unit the literals
// decision (raw or Huffman), then Compressed_Block or Raw_Block.
// tests/test_zstd_huf_host.py builds it with AddressSanitizer and UBSan, runs it as a plain
// program and inflates the frames with libzstd.
//
//   zenc_huf_main <cases.bin> <frame.out>
// cases.bin (little endian): u64 content size, u32 checksum, u32 nblocks, u32 flags (bit 0:
//   Huffman literals), then per block
//   u32 nlit, nlit bytes, u32 nseq, nseq x (u32 ll, u32 ml, u32 off).
// A block is one unit: its source bytes are the literals with the matches copied in (every
// offset points inside the unit).  One line per block goes to stdout:
//   block <type> n <n> nlit <nlit> nseq <nseq> lit <0 raw | 2 huffman> streams <k> sf <f>
//   huf <Huffman section bytes, 0: not eligible> raw <raw section bytes> bits <longest code>
//   last <largest symbol> csz <compressed size>
//
//   zenc_huf_main --lens <hists.bin> <lens.out>
// hists.bin: any number of histograms of 256 u32; lens.out: per histogram u32 longest
//   length (0: not eligible) and 129 u32 code lengths.
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
  std::vector<uint32_t> work(ze::kHufWork);
  for (; at < in.size();) {
    uint32_t hist[256], len[ze::kHufSyms];
    for (uint32_t& h : hist) h = uint32_t(rd(4));
    std::memset(len, 0, sizeof len);
    const uint32_t mb = ze::huf_lengths(hist, len, work.data());
    for (uint32_t i = 0; i <= ze::kHufSyms; ++i) {
      const uint32_t v = i ? len[i - 1] : mb;
      for (int k = 0; k < 4; ++k) out.push_back(uint8_t(v >> (8 * k)));
    }
  }
  return write_file(dst, out) ? 0 : 2;
}

// The Huffman literals section of `lits`, or nothing when they are not eligible by their
// symbols.  The caller compares sizes.
struct HufInfo {
  uint32_t bits = 0, last = 0, streams = 0;
};
static HufInfo huf_section(const uint8_t* lits, uint32_t nlit, std::vector<uint8_t>& sec) {
  HufInfo hi;
  uint32_t hist[256] = {0};
  for (uint32_t i = 0; i < nlit; ++i) hist[lits[i]] += 1;
  std::vector<uint32_t> work(ze::kHufWork);
  uint32_t code[ze::kHufSyms];
  hi.bits = ze::huf_lengths(hist, code, work.data());
  if (!hi.bits) return hi;
  hi.last = ze::huf_codes(code, hi.bits, code, work.data());
  hi.streams = ze::huf_streams(nlit);
  std::vector<uint8_t> body;
  for (uint32_t k = 0; k < ze::huf_tree_size(hi.last); ++k)
    body.push_back(ze::huf_tree_byte(code, hi.bits, hi.last, k));
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
  if (sec.size() != ze::huf_section_size(nlit, hi.last, total)) std::exit(3);
  return hi;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "--lens")) return lens_mode(argv[2], argv[3]);
  if (argc != 3 || !read_file(argv[1])) return 2;

  ze::CTable ct[3];
  for (uint32_t t = 0; t < 3; ++t) ze::build_ctable(ct[t], t);

  const uint64_t fcs = rd(8);
  const uint32_t checksum = uint32_t(rd(4));
  const uint32_t nblocks = uint32_t(rd(4));
  const bool huffman = rd(4) & 1;
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
    if (huffman) hi = huf_section(lits, nlit, huf);
    const uint32_t raw_size = ze::lit_header_size(nlit) + nlit;
    const bool use_huf = hi.bits && huf.size() < raw_size;
    if (hi.bits) {
      const uint32_t streams = uint32_t(huf.size()) - ze::huf_header_size(nlit) -
                               ze::huf_tree_size(hi.last) - (hi.streams == 4 ? 6 : 0);
      if (use_huf != ze::huf_wins(nlit, hi.last, streams)) return 3;
    }
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
    // a unit without sequences is Compressed only with Huffman literals (raw ones are larger)
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
                "last %u csz %u\n",
                comp ? ze::kBlockCompressed : ze::kBlockRaw, n, nlit, nseq,
                hufout ? 2u : 0u, hufout ? hi.streams : 0u,
                hufout ? (hs == 3 ? 0u : hs == 4 ? 2u : 3u) : 0u, huf.size(), raw_size, hi.bits,
                hi.last, csz);
  }
  for (int i = 0; i < 4; ++i) out.push_back(uint8_t(checksum >> (8 * i)));
  if (!write_file(argv[2], out)) return 2;
  std::printf("frame of %zu bytes written\n", out.size());
  return 0;
}
