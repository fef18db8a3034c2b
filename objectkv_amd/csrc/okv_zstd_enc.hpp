// okv_zstd_enc.hpp -- the zstd block encoder's format, stated once (RFC 8878): the
// predefined distributions turned into FSE encode tables, the literal-length /
// match-length / offset codes with their extra bits, the FSE state step, and the
// byte encoders of the frame, block, literals and sequence-count headers.  The device
// encoder (okv_zstd_enc.hip) and tests/zenc_main.cpp on the CPU run these statements.
// Internal header; it includes no HIP header: the functions are __host__ __device__
// when a HIP compiler defines those, plain inline otherwise.
//
// What the encoder emits and nothing else: Raw_Literals_Block, all three sequence
// tables in Predefined_Mode, every offset as Offset_Value = offset + 3 (no repeat
// codes), Raw_Blocks; and under OKV_F_ZSTD_HUFFMAN a Compressed_Literals_Block with
// direct weights where it is smaller, under OKV_F_ZSTD_HUF_FSE with FSE-compressed weights
// too.  Custom FSE tables for the sequences are not here.
#pragma once
#include <cstddef>
#include <cstdint>

#include "okv_sst.h"

#if defined(__host__) && defined(__device__)
#define OKV_ZE_HD __host__ __device__ inline
#else
#define OKV_ZE_HD inline
#endif

namespace okv {
namespace zenc {

constexpr uint32_t kUnit = OKV_ZSTD_ENC_UNIT;  // source bytes per zstd block
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kLL = 0, kML = 1, kOF = 2;  // table order used throughout
constexpr uint32_t kMaxSyms = 53;

OKV_ZE_HD uint32_t highbit(uint32_t v) { return 31u - uint32_t(__builtin_clz(v)); }  // v > 0

// ---- predefined distributions (RFC 8878 3.1.1.3.2.2.1-3) ------------------------
OKV_ZE_HD uint32_t table_log(uint32_t t) { return t == kOF ? 5u : 6u; }
OKV_ZE_HD uint32_t table_syms(uint32_t t) { return t == kLL ? 36u : t == kML ? 53u : 29u; }
OKV_ZE_HD int predefined_norm(uint32_t t, uint32_t s) {
  if (t == kLL) {
    if (s == 0) return 4;
    if (s == 1 || s == 25) return 3;
    if (s >= 32) return -1;
    if ((s >= 13 && s <= 15) || s >= 27) return 1;
    return 2;
  }
  if (t == kML) {
    if (s == 0) return 1;
    if (s == 1) return 4;
    if (s == 2) return 3;
    if (s <= 8) return 2;
    return s >= 46 ? -1 : 1;
  }
  if (s >= 24) return -1;
  return (s >= 6 && s <= 8) ? 2 : 1;
}

// ---- FSE encode table (FSE_buildCTable's construction) ---------------------------
struct CTable {
  uint16_t state[64];      // next-state table, sorted by symbol
  int32_t dfs[kMaxSyms];   // deltaFindState
  uint32_t dnb[kMaxSyms];  // deltaNbBits
  uint32_t log;
};

// From a normalised distribution `norm` of nsym symbols at accuracy `log` (-1: "less than
// one", 0: absent).  sym_at: 2^log bytes, cumul: nsym + 1 entries; the caller says where they
// live (the device passes LDS).
OKV_ZE_HD void build_ctable_norm(CTable& ct, const int32_t* norm, uint32_t nsym, uint32_t log,
                                 uint8_t* sym_at, uint16_t* cumul) {
  const uint32_t size = 1u << log, mask = size - 1;
  const uint32_t step = (size >> 1) + (size >> 3) + 3;
  uint32_t high = size - 1;
  cumul[0] = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    const int nrm = norm[s];
    if (nrm == -1) {
      cumul[s + 1] = uint16_t(cumul[s] + 1);
      sym_at[high--] = uint8_t(s);
    } else {
      cumul[s + 1] = uint16_t(cumul[s] + nrm);
    }
  }
  uint32_t pos = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    const int nrm = norm[s];
    for (int i = 0; i < nrm; ++i) {
      sym_at[pos] = uint8_t(s);
      pos = (pos + step) & mask;
      while (pos > high) pos = (pos + step) & mask;
    }
  }
  for (uint32_t u = 0; u < size; ++u) ct.state[cumul[sym_at[u]]++] = uint16_t(size + u);
  uint32_t total = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    const int nrm = norm[s];
    if (nrm == 0) {  // never coded
      ct.dnb[s] = ((log + 1) << 16) - size;
      ct.dfs[s] = 0;
    } else if (nrm == -1 || nrm == 1) {
      ct.dnb[s] = (log << 16) - size;
      ct.dfs[s] = int32_t(total) - 1;
      total += 1;
    } else {
      const uint32_t max_bits = log - highbit(uint32_t(nrm) - 1);
      ct.dnb[s] = (max_bits << 16) - (uint32_t(nrm) << max_bits);
      ct.dfs[s] = int32_t(total) - nrm;
      total += uint32_t(nrm);
    }
  }
  ct.log = log;
}
// The predefined table t.
OKV_ZE_HD void build_ctable(CTable& ct, uint32_t t) {
  int32_t norm[kMaxSyms];
  uint8_t sym_at[64];
  uint16_t cumul[kMaxSyms + 1];
  const uint32_t nsym = table_syms(t);
  for (uint32_t s = 0; s < nsym; ++s) norm[s] = predefined_norm(t, s);
  build_ctable_norm(ct, norm, nsym, table_log(t), sym_at, cumul);
}

// The state a chain starts in (FSE_initCState2): the symbol of the LAST sequence.
OKV_ZE_HD uint32_t fse_init(const CTable& ct, uint32_t sym) {
  const uint32_t dnb = ct.dnb[sym];
  const uint32_t nb = (dnb + (1u << 15)) >> 16;
  const uint32_t value = (nb << 16) - dnb;
  return ct.state[int32_t(value >> nb) + ct.dfs[sym]];
}
// One step (FSE_encodeSymbol): the low nb bits of the state go out, then the state moves.
OKV_ZE_HD uint32_t fse_step(const CTable& ct, uint32_t state, uint32_t sym, uint32_t& nb,
                            uint32_t& bits) {
  nb = (state + ct.dnb[sym]) >> 16;
  bits = state & ((1u << nb) - 1);
  return ct.state[int32_t(state >> nb) + ct.dfs[sym]];
}

// ---- codes and extra bits (RFC 8878 3.1.1.3.2.1.1) -------------------------------
OKV_ZE_HD uint32_t ll_code(uint32_t ll) {
  if (ll < 16) return ll;
  if (ll < 24) return 16 + ((ll - 16) >> 1);
  if (ll < 32) return 20 + ((ll - 24) >> 2);
  if (ll < 48) return 22 + ((ll - 32) >> 3);
  if (ll < 64) return 24;
  return highbit(ll) + 19;
}
OKV_ZE_HD uint32_t ll_bits(uint32_t c) {
  return c < 16 ? 0 : c < 20 ? 1 : c < 22 ? 2 : c < 24 ? 3 : c == 24 ? 4 : c == 25 ? 6 : c - 19;
}
OKV_ZE_HD uint32_t ll_base(uint32_t c) {
  if (c < 16) return c;
  if (c < 20) return 16 + 2 * (c - 16);
  if (c < 22) return 24 + 4 * (c - 20);
  if (c < 24) return 32 + 8 * (c - 22);
  if (c == 24) return 48;
  return 1u << (c - 19);
}
// match lengths are coded as ml - 3 ("mb" below)
OKV_ZE_HD uint32_t ml_code(uint32_t mb) {
  if (mb < 32) return mb;
  if (mb < 40) return 32 + ((mb - 32) >> 1);
  if (mb < 48) return 36 + ((mb - 40) >> 2);
  if (mb < 64) return 38 + ((mb - 48) >> 3);
  if (mb < 96) return 40 + ((mb - 64) >> 4);
  if (mb < 128) return 42;
  return highbit(mb) + 36;
}
OKV_ZE_HD uint32_t ml_bits(uint32_t c) {
  return c < 32 ? 0 : c < 36 ? 1 : c < 38 ? 2 : c < 40 ? 3 : c < 42 ? 4 : c == 42 ? 5 : c - 36;
}
OKV_ZE_HD uint32_t ml_base(uint32_t c) {  // of ml - 3
  if (c < 32) return c;
  if (c < 36) return 32 + 2 * (c - 32);
  if (c < 38) return 40 + 4 * (c - 36);
  if (c < 40) return 48 + 8 * (c - 38);
  if (c < 42) return 64 + 16 * (c - 40);
  if (c == 42) return 96;
  return 1u << (c - 36);
}

// One sequence as the bitstream wants it: three symbols, and per field the number of
// extra bits and their value.  off is the match distance (>= 1); it is always coded as
// Offset_Value = off + 3, so no repeat-offset history exists on either side.
struct SeqCode {
  uint32_t sym[3];  // kLL, kML, kOF
  uint32_t xb[3];   // extra bit counts
  uint32_t xv[3];   // extra bit values
};
OKV_ZE_HD SeqCode seq_code(uint32_t ll, uint32_t ml, uint32_t off) {
  SeqCode c;
  c.sym[kLL] = ll_code(ll);
  c.xb[kLL] = ll_bits(c.sym[kLL]);
  c.xv[kLL] = ll - ll_base(c.sym[kLL]);
  const uint32_t mb = ml - 3;
  c.sym[kML] = ml_code(mb);
  c.xb[kML] = ml_bits(c.sym[kML]);
  c.xv[kML] = mb - ml_base(c.sym[kML]);
  const uint32_t ov = off + 3;
  c.sym[kOF] = highbit(ov);
  c.xb[kOF] = c.sym[kOF];
  c.xv[kOF] = ov - (1u << c.sym[kOF]);
  return c;
}
// The symbol alone, for a state chain that walks one table.
OKV_ZE_HD uint32_t seq_sym(uint32_t t, uint32_t ll, uint32_t ml, uint32_t off) {
  return t == kLL ? ll_code(ll) : t == kML ? ml_code(ml - 3) : highbit(off + 3);
}

// The bits one sequence adds, in stream order (low bits first), as zstd's
// ZSTD_encodeSequences adds them: for every sequence but the last the three state
// steps -- offset, match length, literal length -- and then for every sequence the
// extra bits: literal length, match length, offset.  `st` holds the (nb, bits) each
// chain's step gave for this sequence (nb = 0 for the last sequence, whose symbols
// the chains start from).  At most 17 + 16 + 16 + 28 bits: two words.
struct SeqBits {
  uint64_t lo, hi;  // hi is used only past 64 bits
  uint32_t nb;
};
OKV_ZE_HD void bits_push(SeqBits& b, uint64_t v, uint32_t n) {
  if (!n) return;
  if (b.nb < 64) {
    b.lo |= v << b.nb;
    if (b.nb + n > 64) b.hi |= v >> (64 - b.nb);
  } else {
    b.hi |= v << (b.nb - 64);
  }
  b.nb += n;
}
OKV_ZE_HD SeqBits seq_bits(const SeqCode& c, const uint32_t st_nb[3], const uint32_t st_bits[3]) {
  SeqBits b = {0, 0, 0};
  bits_push(b, st_bits[kOF], st_nb[kOF]);
  bits_push(b, st_bits[kML], st_nb[kML]);
  bits_push(b, st_bits[kLL], st_nb[kLL]);
  bits_push(b, c.xv[kLL], c.xb[kLL]);
  bits_push(b, c.xv[kML], c.xb[kML]);
  bits_push(b, c.xv[kOF], c.xb[kOF]);
  return b;
}
// What closes the stream after the first sequence's bits: the final states, match
// length, offset, literal length, each in its table's log bits, then the end mark.
OKV_ZE_HD SeqBits close_bits(const uint32_t fin[3]) {
  SeqBits b = {0, 0, 0};
  bits_push(b, fin[kML] & 63u, 6);
  bits_push(b, fin[kOF] & 31u, 5);
  bits_push(b, fin[kLL] & 63u, 6);
  bits_push(b, 1, 1);
  return b;
}

// ---- header bytes ----------------------------------------------------------------
// Frame header: magic, Single_Segment, Content_Checksum, no dictionary, and
// Frame_Content_Size in the smallest field that holds it.  Returns its length (6..13).
OKV_ZE_HD uint32_t frame_header_size(uint64_t fcs) {
  return 5 + (fcs < 256 ? 1 : fcs < 65792 ? 2 : fcs < (uint64_t(1) << 32) ? 4 : 8);
}
OKV_ZE_HD uint32_t frame_header(uint8_t* p, uint64_t fcs) {
  const uint32_t flag = fcs < 256 ? 0 : fcs < 65792 ? 1 : fcs < (uint64_t(1) << 32) ? 2 : 3;
  const uint32_t nb = flag == 0 ? 1 : flag == 1 ? 2 : flag == 2 ? 4 : 8;
  const uint64_t v = flag == 1 ? fcs - 256 : fcs;
  p[0] = 0x28, p[1] = 0xB5, p[2] = 0x2F, p[3] = 0xFD;
  p[4] = uint8_t((flag << 6) | (1u << 5) | (1u << 2));
  for (uint32_t i = 0; i < nb; ++i) p[5 + i] = uint8_t(v >> (8 * i));
  return 5 + nb;
}
constexpr uint32_t kBlockRaw = 0, kBlockRle = 1, kBlockCompressed = 2;
OKV_ZE_HD void block_header(uint8_t* p, bool last, uint32_t type, uint32_t size) {
  const uint32_t v = (last ? 1u : 0u) | (type << 1) | (size << 3);
  p[0] = uint8_t(v), p[1] = uint8_t(v >> 8), p[2] = uint8_t(v >> 16);
}
// Raw_Literals_Block header: the 1-, 2- and 3-byte size formats.
OKV_ZE_HD uint32_t lit_header_size(uint32_t n) { return n < 32 ? 1 : n < 4096 ? 2 : 3; }
OKV_ZE_HD uint32_t lit_header(uint8_t* p, uint32_t n) {
  if (n < 32) {
    p[0] = uint8_t(n << 3);
    return 1;
  }
  if (n < 4096) {
    const uint32_t v = (n << 4) | (1u << 2);
    p[0] = uint8_t(v), p[1] = uint8_t(v >> 8);
    return 2;
  }
  const uint32_t v = (n << 4) | (3u << 2);
  p[0] = uint8_t(v), p[1] = uint8_t(v >> 8), p[2] = uint8_t(v >> 16);
  return 3;
}
// Number_of_Sequences: 1 byte below 128, 2 bytes below 0x7F00, else 3.
OKV_ZE_HD uint32_t nseq_header_size(uint32_t n) { return n < 128 ? 1 : n < 0x7F00 ? 2 : 3; }
OKV_ZE_HD uint32_t nseq_header(uint8_t* p, uint32_t n) {
  if (n < 128) {
    p[0] = uint8_t(n);
    return 1;
  }
  if (n < 0x7F00) {
    p[0] = uint8_t((n >> 8) + 128), p[1] = uint8_t(n);
    return 2;
  }
  p[0] = 255, p[1] = uint8_t(n - 0x7F00), p[2] = uint8_t((n - 0x7F00) >> 8);
  return 3;
}
// A Compressed_Block's size from its parts; the bitstream carries `bits` sequence bits
// (close_bits included), rounded up to bytes.
OKV_ZE_HD uint32_t compressed_size(uint32_t nlit, uint32_t nseq, uint64_t bits) {
  return lit_header_size(nlit) + nlit + nseq_header_size(nseq) + 1 + uint32_t((bits + 7) >> 3);
}
// A block's size from the size of its literals section (raw or Huffman) and its sequences.
// Without sequences the sequences section is the single byte 0.
OKV_ZE_HD uint32_t block_content_size(uint32_t litsec, uint32_t nseq, uint64_t bits) {
  return litsec + nseq_header_size(nseq) + (nseq ? 1 + uint32_t((bits + 7) >> 3) : 0);
}

// ---- Huffman-coded literals (OKV_F_ZSTD_HUFFMAN; RFC 8878 3.1.1.3.1, 4.2) ---------
// A unit's literals become a Compressed_Literals_Block only if at least two byte values
// occur, none is above kHufMaxSym (the tree description lists direct 4-bit weights: header
// byte 127 + number of listed weights, and 255 - 127 = 128 listed weights describe the
// symbols 0 .. 128), and the section is strictly smaller than the raw one.  Code lengths
// are the length-limited optimum of package-merge at kHufMaxBits; weights, the canonical
// codes and the stream split are the RFC's.  FSE-compressed weights and values above
// kHufMaxSym come with OKV_F_ZSTD_HUF_FSE (below); no RLE and no treeless literals.
constexpr uint32_t kHufMaxBits = 11;
constexpr uint32_t kHufMaxSym = 128;
constexpr uint32_t kHufSyms = kHufMaxSym + 1;
constexpr uint32_t kHufItems = 2 * kHufSyms - 2;  // items package-merge keeps per level
// Words of work space huf_lengths needs: the sorted leaves, two item lists, one flag
// byte per item and level.
constexpr uint32_t kHufWork = kHufSyms + 2 * kHufItems + kHufMaxBits * kHufItems / 4;
static_assert(kHufItems % 4 == 0, "a level's flag bytes are whole words");
// The same sizes for any symbol limit: the item lists and a level's flag bytes keep a stride
// of whole words (2 * 256 - 2 = 510 items are padded to 512).
template <uint32_t MAXSYM>
struct HufDim {
  static constexpr uint32_t syms = MAXSYM + 1;
  static constexpr uint32_t items = 2 * syms - 2;
  static constexpr uint32_t stride = (items + 3) & ~3u;
  static constexpr uint32_t work = syms + 2 * stride + kHufMaxBits * stride / 4;
};
constexpr uint32_t kHufAllSyms = 256;  // OKV_F_ZSTD_HUF_FSE: every byte value may have a code
constexpr uint32_t kHufAllWork = HufDim<kHufAllSyms - 1>::work;
static_assert(HufDim<kHufMaxSym>::work == kHufWork && HufDim<kHufMaxSym>::stride == kHufItems,
              "the direct-weights instance is the one stated above");

// Code lengths from a histogram of 256 counts (their sum below 2^23): len[s] for
// s <= kHufMaxSym, 0 for an absent symbol.  Returns the longest length, or 0 when the
// literals are not eligible (fewer than two distinct values, or a value above kHufMaxSym;
// len is then not meaningful).  Package-merge (Larmore and Hirschberg): level 0 is the
// leaves in order of (count, symbol); a level is the leaves merged with the pairs of the
// level below, a leaf before a package of equal weight; the first 2n - 2 items of the last
// level are taken, and going down, twice as many items as packages were taken above.  A
// leaf's length is the number of levels that took it.
template <uint32_t MAXSYM>
OKV_ZE_HD uint32_t huf_lengths_n(const uint32_t* hist, uint32_t* len, uint32_t* work) {
  constexpr uint32_t kSyms = HufDim<MAXSYM>::syms, kStride = HufDim<MAXSYM>::stride;
  uint32_t* key = work;                    // (count << 8) | symbol, ascending
  uint32_t* cur = work + kSyms;            // item weights of the level being built
  uint32_t* prev = cur + kStride;          // ... of the level below
  uint8_t* flag = reinterpret_cast<uint8_t*>(prev + kStride);  // 1: the item is a package
  uint32_t n = 0;
  for (uint32_t s = kSyms; s < 256; ++s)  // (first: the common way out)
    if (hist[s]) return 0;
  for (uint32_t s = 0; s < kSyms; ++s) {
    const uint32_t c = hist[s];
    if (!c) continue;
    uint32_t i = n++;  // insertion: counts ascending, equal counts by symbol
    const uint32_t k = (c << 8) | s;
    for (; i > 0 && key[i - 1] > k; --i) key[i] = key[i - 1];
    key[i] = k;
  }
  if (n < 2) return 0;
  const uint32_t keep = 2 * n - 2;
  // no code of n symbols is deeper than n - 1: fewer levels give the same lengths' cost
  const uint32_t levels = n - 1 < kHufMaxBits ? n - 1 : kHufMaxBits;
  for (uint32_t i = 0; i < n; ++i) prev[i] = key[i] >> 8;
  uint32_t plen = n;
  for (uint32_t lv = 1; lv < levels; ++lv) {
    uint8_t* fl = flag + lv * kStride;
    const uint32_t np = plen / 2;
    uint32_t i = 0, j = 0, cnt = 0;
    while (cnt < keep && (i < n || j < np)) {
      const uint32_t wl = i < n ? key[i] >> 8 : 0xFFFFFFFFu;
      const uint32_t wp = j < np ? prev[2 * j] + prev[2 * j + 1] : 0xFFFFFFFFu;
      const bool leaf = i < n && wl <= wp;
      cur[cnt] = leaf ? wl : wp;
      fl[cnt] = leaf ? 0 : 1;
      i += leaf ? 1 : 0;
      j += leaf ? 0 : 1;
      ++cnt;
    }
    plen = cnt;
    uint32_t* t = cur;
    cur = prev;
    prev = t;
  }
  // (a complete code of n <= 2^levels leaves exists: the last level holds `keep` items)
  uint32_t* depth = cur;  // per sorted leaf; the item lists are done with
  for (uint32_t i = 0; i < n; ++i) depth[i] = 0;
  uint32_t take = keep < plen ? keep : plen;
  for (uint32_t lv = levels; lv-- > 0 && take;) {
    uint32_t packs = 0;
    if (lv) {
      const uint8_t* fl = flag + lv * kStride;
      for (uint32_t i = 0; i < take; ++i) packs += fl[i];
    }
    const uint32_t leaves = take - packs;
    for (uint32_t i = 0; i < leaves; ++i) depth[i] += 1;
    take = 2 * packs;
  }
  for (uint32_t s = 0; s < kSyms; ++s) len[s] = 0;
  for (uint32_t i = 0; i < n; ++i) len[key[i] & 255u] = depth[i];
  return depth[0];
}
OKV_ZE_HD uint32_t huf_lengths(const uint32_t* hist, uint32_t* len, uint32_t* work) {
  return huf_lengths_n<kHufMaxSym>(hist, len, work);
}
// The same over all 256 byte values (OKV_F_ZSTD_HUF_FSE); work: kHufAllWork words.  Without a
// value above kHufMaxSym the keys, their order and so the lengths are huf_lengths'.
OKV_ZE_HD uint32_t huf_lengths_all(const uint32_t* hist, uint32_t* len, uint32_t* work) {
  return huf_lengths_n<kHufAllSyms - 1>(hist, len, work);
}

// The canonical codes (RFC 8878 4.2.1.3, HUF_buildCTable's order): the longest codes start
// at 0 and count up by symbol value; a shorter length starts at half of where the longer
// ones ended.  code[s] = (value << 4) | length, 0 for an absent symbol; `len` and `code`
// may be the same array.  Returns the largest present symbol.  work: 32 words.
template <uint32_t NSYM>
OKV_ZE_HD uint32_t huf_codes_n(const uint32_t* len, uint32_t max_bits, uint32_t* code,
                               uint32_t* work) {
  uint32_t* per = work;       // symbols per length
  uint32_t* val = work + 16;  // next value per length
  for (uint32_t b = 0; b < 16; ++b) per[b] = 0;
  uint32_t last = 0;
  for (uint32_t s = 0; s < NSYM; ++s)
    if (len[s]) per[len[s]] += 1, last = s;
  uint32_t min = 0;
  for (uint32_t b = max_bits; b > 0; --b) {
    val[b] = min;
    min = (min + per[b]) >> 1;
  }
  for (uint32_t s = 0; s < NSYM; ++s) {
    const uint32_t b = len[s];
    code[s] = b ? ((val[b]++) << 4) | b : 0;
  }
  return last;
}
OKV_ZE_HD uint32_t huf_codes(const uint32_t* len, uint32_t max_bits, uint32_t* code,
                             uint32_t* work) {
  return huf_codes_n<kHufSyms>(len, max_bits, code, work);
}
OKV_ZE_HD uint32_t huf_codes_all(const uint32_t* len, uint32_t max_bits, uint32_t* code,
                                 uint32_t* work) {
  return huf_codes_n<kHufAllSyms>(len, max_bits, code, work);
}
// The weight the tree description lists for a code of `bits` bits (0: absent).
OKV_ZE_HD uint32_t huf_weight(uint32_t bits, uint32_t max_bits) {
  return bits ? max_bits + 1 - bits : 0;
}
// Tree description: header byte, then the weights of the symbols below `last` (the
// largest present one, whose weight is implied), two a byte, high nibble first.
OKV_ZE_HD uint32_t huf_tree_size(uint32_t last) { return 1 + (last + 1) / 2; }
OKV_ZE_HD uint8_t huf_tree_byte(const uint32_t* code, uint32_t max_bits, uint32_t last,
                                uint32_t k) {  // byte k of the description, k < huf_tree_size
  if (k == 0) return uint8_t(127 + last);
  const uint32_t s = 2 * (k - 1);
  const uint32_t hi = huf_weight(code[s] & 15u, max_bits);
  const uint32_t lo = s + 1 < last ? huf_weight(code[s + 1] & 15u, max_bits) : 0;
  return uint8_t((hi << 4) | lo);
}
// One stream up to 1 023 literals, else four: the first three of (nlit + 3) / 4 literals.
OKV_ZE_HD uint32_t huf_streams(uint32_t nlit) { return nlit <= 1023 ? 1u : 4u; }
OKV_ZE_HD uint32_t huf_stream_len(uint32_t nlit, uint32_t s) {
  if (nlit <= 1023) return nlit;
  const uint32_t seg = (nlit + 3) / 4;
  return s < 3 ? seg : nlit - 3 * seg;
}
// A stream of `bits` code bits: the end mark, padded to a byte.
OKV_ZE_HD uint32_t huf_stream_bytes(uint32_t bits) { return (bits + 1 + 7) >> 3; }
// Compressed_Literals_Block header: Size_Format 00 (one stream, 10-bit sizes), 10 (14 bits)
// or 11 (18 bits); 01 is never written.  `comp` counts the tree description, the jump
// table and the streams.
OKV_ZE_HD uint32_t huf_header_size(uint32_t nlit) { return nlit <= 1023 ? 3 : nlit <= 16383 ? 4 : 5; }
OKV_ZE_HD uint32_t huf_header(uint8_t* p, uint32_t nlit, uint32_t comp) {
  const uint32_t hs = huf_header_size(nlit);
  const uint32_t sf = hs == 3 ? 0 : hs == 4 ? 2 : 3, sb = hs == 3 ? 10 : hs == 4 ? 14 : 18;
  const uint64_t v = 2u | (sf << 2) | (uint64_t(nlit) << 4) | (uint64_t(comp) << (4 + sb));
  for (uint32_t i = 0; i < hs; ++i) p[i] = uint8_t(v >> (8 * i));
  return hs;
}
// The section's size from the sum of its streams' bytes.
OKV_ZE_HD uint32_t huf_section_size(uint32_t nlit, uint32_t last, uint32_t stream_bytes) {
  return huf_header_size(nlit) + huf_tree_size(last) + (huf_streams(nlit) == 4 ? 6 : 0) +
         stream_bytes;
}
// The rule: Huffman only when strictly smaller than the raw section.
OKV_ZE_HD bool huf_wins(uint32_t nlit, uint32_t last, uint32_t stream_bytes) {
  return huf_section_size(nlit, last, stream_bytes) < lit_header_size(nlit) + nlit;
}

// ---- FSE-compressed weights (OKV_F_ZSTD_HUF_FSE; RFC 8878 4.2.1.2) -----------------
// The second form of the tree description: header byte = its compressed size (< 128), an
// NCount header, and the weights of the symbols 0 .. last-1 (values 0 .. kHufMaxBits)
// through two interleaved FSE states, written backwards.  It exists when there are at least
// two listed weights, they are not all one value and it takes at most kWtMaxBytes bytes.
// It is used iff it exists and is strictly smaller than the direct one, or the direct one
// does not exist (last > kHufMaxSym); a tie goes to direct.
constexpr uint32_t kWtSyms = kHufMaxBits + 1;  // weight values
constexpr uint32_t kWtMaxBytes = 127;
// The accuracy log (the decoders take 5 or 6): 6 from 128 listed weights on, else 5.  A
// finer table pays only when many weights share its header.
OKV_ZE_HD uint32_t wt_log(uint32_t listed) { return listed >= 128 ? 6u : 5u; }

// Everything the description needs besides registers; the device keeps it in LDS.
struct WtWork {
  CTable ct;
  int32_t norm[kWtSyms];
  uint32_t cnt[kWtSyms];
  uint16_t cumul[kWtSyms + 2];
  uint8_t sym_at[64];
  uint8_t w[256];    // the listed weights
  uint8_t st[256];   // per weight: (1 << nb) | bits of its state step
  uint8_t out[128];  // NCount header, then the stream
  uint32_t fin[2];   // the chains' final states
};
static_assert(sizeof(WtWork) % 4 == 0, "whole words of LDS");

// Normalised counts summing to 2^log: each present value gets its share rounded to nearest,
// at least 1; what is missing goes to the most frequent value (the lowest on a tie), what is
// too much is taken one at a time from the value that holds most.  Returns the number of
// values up to the largest present one, or 0 when all weights are one value.
OKV_ZE_HD uint32_t wt_normalise(const uint32_t* cnt, uint32_t total, uint32_t log, int32_t* norm) {
  const uint32_t size = 1u << log;
  uint32_t nsym = 0, sum = 0, big = 0;
  for (uint32_t s = 0; s < kWtSyms; ++s) {
    const uint32_t c = cnt[s];
    if (c == total) return 0;
    uint32_t p = c ? (c * size + total / 2) / total : 0;
    if (c && !p) p = 1;
    norm[s] = int32_t(p);
    sum += p;
    if (c) nsym = s + 1;
    if (cnt[s] > cnt[big]) big = s;
  }
  if (sum <= size) {
    norm[big] += int32_t(size - sum);
  } else {
    for (uint32_t over = sum - size; over; --over) {  // (at most kWtSyms: each rounds up < 1)
      uint32_t m = 0;
      for (uint32_t s = 1; s < kWtSyms; ++s)
        if (norm[s] > norm[m]) m = s;
      norm[m] -= 1;  // (it holds at least 3: more than 2^log >= 32 is spread over 12 values)
    }
  }
  return nsym;
}

// The NCount header (RFC 8878 4.1.1) of norm[0 .. nsym): 4 bits of log - 5, then every count
// as count + 1 in the fewest bits the rest still to give allows (the low values of the range
// take one bit less), and after a zero the number of further zeros in 2-bit groups.  Bits go
// low first.  At most 4 + 12 * 7 + 12 bits.  Returns its bytes.
OKV_ZE_HD uint32_t wt_ncount(const int32_t* norm, uint32_t nsym, uint32_t log, uint8_t* out) {
  SeqBits b = {0, 0, 0};
  bits_push(b, log - 5, 4);
  int32_t remaining = int32_t(1u << log) + 1, threshold = int32_t(1u << log);
  uint32_t nb = log + 1, s = 0;
  bool zero = false;
  while (s < nsym && remaining > 1) {
    if (zero) {
      uint32_t start = s;
      while (s < nsym && !norm[s]) ++s;  // (norm[nsym - 1] is not 0)
      for (; s >= start + 3; start += 3) bits_push(b, 3, 2);
      bits_push(b, s - start, 2);
    }
    int32_t v = norm[s++];
    const int32_t max = 2 * threshold - 1 - remaining;
    remaining -= v;
    v += 1;
    if (v >= threshold) v += max;
    bits_push(b, uint32_t(v), nb - (v < max ? 1u : 0u));
    zero = v == 1;
    while (remaining < threshold && threshold > 1) --nb, threshold >>= 1;
  }
  const uint32_t bytes = (b.nb + 7) >> 3;
  for (uint32_t i = 0; i < bytes; ++i)
    out[i] = uint8_t(i < 8 ? b.lo >> (8 * i) : b.hi >> (8 * (i - 8)));
  return bytes;
}

// Step one, by one lane: the histogram of the n listed weights w.w[0 .. n), their norm, the
// header into w.out and the encode table.  Returns the header's bytes, 0 when there is no
// FSE description.
OKV_ZE_HD uint32_t wt_prepare(WtWork& w, uint32_t n) {
  if (n < 2) return 0;
  for (uint32_t s = 0; s < kWtSyms; ++s) w.cnt[s] = 0;
  for (uint32_t i = 0; i < n; ++i) w.cnt[w.w[i]] += 1;
  const uint32_t log = wt_log(n);
  const uint32_t nsym = wt_normalise(w.cnt, n, log, w.norm);
  if (!nsym) return 0;
  build_ctable_norm(w.ct, w.norm, nsym, log, w.sym_at, w.cumul);
  return wt_ncount(w.norm, nsym, log, w.out);
}
// Step two, chain p of two (they are independent): the weights at the indices of parity p,
// last to first.  The last such weight starts the state and costs no bits.  Weight 0 is the
// first symbol the decoder reads, from the state that is flushed last: chain 0.
OKV_ZE_HD void wt_chain(WtWork& w, uint32_t n, uint32_t p) {
  uint32_t i = n - 1 - ((n - 1 - p) & 1u);
  uint32_t state = fse_init(w.ct, w.w[i]);
  w.st[i] = 1;
  while (i >= 2) {
    i -= 2;
    uint32_t nb, bits;
    state = fse_step(w.ct, state, w.w[i], nb, bits);
    w.st[i] = uint8_t((1u << nb) | bits);
  }
  w.fin[p] = state;
}
// Step three: the steps' bits from the last weight to the first, the final states (chain 1,
// then chain 0, log bits each) and the end mark, behind the `nc` header bytes.  Returns the
// description's bytes without its header byte, 0 when they are more than kWtMaxBytes.
OKV_ZE_HD uint32_t wt_pack(WtWork& w, uint32_t n, uint32_t nc) {
  const uint32_t log = w.ct.log, mask = (1u << log) - 1;
  uint64_t acc = 0;
  uint32_t an = 0, at = nc;
  const auto add = [&](uint32_t v, uint32_t nb) {
    acc |= uint64_t(v) << an;
    an += nb;
    for (; an >= 8; an -= 8, acc >>= 8, ++at)
      if (at < kWtMaxBytes) w.out[at] = uint8_t(acc);
  };
  for (uint32_t i = n; i-- > 0;) {
    const uint32_t e = w.st[i], nb = highbit(e);
    add(e - (1u << nb), nb);
  }
  add(w.fin[1] & mask, log);
  add(w.fin[0] & mask, log);
  add(1, 8 - an % 8);  // (the end mark and zeros up to the byte)
  return at <= kWtMaxBytes ? at : 0;
}

// Which description: its bytes with the header byte, 0 when there is none (the literals stay
// raw).  fse_bytes: wt_pack's result.
OKV_ZE_HD uint32_t huf_desc_size(uint32_t last, uint32_t fse_bytes, bool& fse) {
  const uint32_t direct = last <= kHufMaxSym ? huf_tree_size(last) : 0;
  fse = fse_bytes && (!direct || 1 + fse_bytes < direct);
  return fse ? 1 + fse_bytes : direct;
}
// huf_section_size and huf_wins from the description's bytes.
OKV_ZE_HD uint32_t huf_section_size_d(uint32_t nlit, uint32_t desc, uint32_t stream_bytes) {
  return huf_header_size(nlit) + desc + (huf_streams(nlit) == 4 ? 6 : 0) + stream_bytes;
}
OKV_ZE_HD bool huf_wins_d(uint32_t nlit, uint32_t desc, uint32_t stream_bytes) {
  return huf_section_size_d(nlit, desc, stream_bytes) < lit_header_size(nlit) + nlit;
}

// Upper bound of a frame for `orig` raw bytes: every unit a Raw_Block.
OKV_ZE_HD uint64_t frame_bound(uint64_t orig) {
  const uint64_t units = orig ? (orig + kUnit - 1) / kUnit : 1;
  return orig + 3 * units + 18;
}

}  // namespace zenc
}  // namespace okv
