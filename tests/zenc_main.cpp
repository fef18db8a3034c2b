// zenc_main.cpp -- writes one zstd frame from literals and sequence lists using only
// objectkv_amd/csrc/okv_zstd_enc.hpp (the statements the device encoder runs), with the
// sequence bits placed one after another.  tests/test_zstd_enc_host.py builds it with
// AddressSanitizer and UBSan, runs it as a plain program and inflates the frame with
// libzstd.
//
//   zenc_main <cases.bin> <frame.out>
// cases.bin (little endian): u64 content size, u32 checksum, u32 nblocks, then per block
//   u32 nlit, nlit bytes, u32 nseq, nseq x (u32 ll, u32 ml, u32 off).
// A block without sequences becomes a Raw_Block of its literals.
#include <cstdio>
#include <cstdlib>
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

static void put(std::vector<uint8_t>& out, const uint8_t* p, uint32_t n) {
  out.insert(out.end(), p, p + n);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  for (int c; (c = std::fgetc(f)) != EOF;) in.push_back(uint8_t(c));
  std::fclose(f);

  ze::CTable ct[3];
  for (uint32_t t = 0; t < 3; ++t) ze::build_ctable(ct[t], t);

  const uint64_t fcs = rd(8);
  const uint32_t checksum = uint32_t(rd(4));
  const uint32_t nblocks = uint32_t(rd(4));
  std::vector<uint8_t> out;
  uint8_t hb[16];
  put(out, hb, ze::frame_header(hb, fcs));
  if (ze::frame_header_size(fcs) != out.size()) return 3;
  for (uint32_t b = 0; b < nblocks; ++b) {
    const uint32_t nlit = uint32_t(rd(4));
    if (at + nlit > in.size()) return 2;
    const uint8_t* lits = in.data() + at;
    at += nlit;
    const uint32_t nseq = uint32_t(rd(4));
    std::vector<Seq> seqs(nseq);
    for (Seq& s : seqs) s.ll = uint32_t(rd(4)), s.ml = uint32_t(rd(4)), s.off = uint32_t(rd(4));
    const bool last = b + 1 == nblocks;
    const size_t head = out.size();
    out.resize(head + 3);
    if (!nseq) {
      ze::block_header(out.data() + head, last, ze::kBlockRaw, nlit);
      put(out, lits, nlit);
      continue;
    }
    put(out, hb, ze::lit_header(hb, nlit));
    put(out, lits, nlit);
    put(out, hb, ze::nseq_header(hb, nseq));
    out.push_back(0);  // Predefined_Mode for all three tables
    const size_t stream_at = out.size();
    BitWriter bw(out);
    uint32_t state[3];
    for (uint32_t t = 0; t < 3; ++t) {
      const Seq& s = seqs[nseq - 1];
      state[t] = ze::fse_init(ct[t], ze::seq_sym(t, s.ll, s.ml, s.off));
    }
    for (uint32_t k = nseq; k-- > 0;) {
      const Seq& s = seqs[k];
      const ze::SeqCode c = ze::seq_code(s.ll, s.ml, s.off);
      uint32_t nb[3] = {0, 0, 0}, bits[3] = {0, 0, 0};
      if (k + 1 != nseq)
        for (uint32_t t = 0; t < 3; ++t) {
          if (c.sym[t] != ze::seq_sym(t, s.ll, s.ml, s.off)) return 3;
          state[t] = ze::fse_step(ct[t], state[t], c.sym[t], nb[t], bits[t]);
        }
      bw.add(ze::seq_bits(c, nb, bits));
    }
    bw.add(ze::close_bits(state));
    const size_t size = out.size() - head - 3;
    if (size != ze::compressed_size(nlit, nseq, bw.nbits) || out.size() - stream_at == 0) return 3;
    ze::block_header(out.data() + head, last, ze::kBlockCompressed, uint32_t(size));
  }
  for (int i = 0; i < 4; ++i) out.push_back(uint8_t(checksum >> (8 * i)));
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(out.data(), 1, out.size(), f);
  std::fclose(f);
  std::printf("frame of %zu bytes written\n", out.size());
  return 0;
}
