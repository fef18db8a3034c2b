// okv_zstd_enc.hip -- the zstd block encoder on the device (OKV_F_ZSTD_NATIVE).
//
// okv_encode.hip cuts the rows into blocks and packs each block's records contiguously
// into a scratch image (its own cut and pack kernels, at a 16-byte padding unit).  This
// file turns every block of that image into one RFC 8878 frame and lays the frames out
// as the Go writer lays out compressed blocks:
//   Z1 okv_zenc_plan_kernel   units per block (kUnit source bytes each), their prefix, and
//                             the size bound from the raw sizes alone (the capacity contract)
//   Z2 okv_zenc_unit_kernel   one workgroup per unit: match, parse, sequence coding; the
//                             unit's zstd block (Compressed or Raw) into its scratch slot
//                             (the encode tables: okv_zenc_tables_kernel, once per context)
//   Z3 okv_hash_kernel        XXH64 of each raw block (the frame's Content_Checksum)
//   Z4 okv_zenc_size_kernel   CompressedSize, BlockSize (Q2), Offset, the units' places
//   Z5 okv_zenc_place_kernel  header, units, checksum and zero padding into the segment,
//                             16 bytes per store
//   Z6 okv_hash_kernel        BlockStat.Hash over each padded block
// The format statements (tables, codes, state step, header bytes) are okv_zstd_enc.hpp's,
// which tests/zenc_main.cpp runs on the CPU.
//
// Z2's LDS, one workgroup of 256 threads per CU (160 500 of the CU's 163 840 bytes, so one
// wave per SIMD): the unit (32 KiB + a line before and two after), one u16 per position
// (its hash, then its candidate, then -- behind the parse -- the sequences), the hash
// table of 2^14 u16 entries (later the bitstream words) and one byte per sequence and
// state chain.
#include "okv_ctx.hpp"
#include "okv_zstd_enc.hpp"

namespace okv {
namespace zenc {

constexpr uint32_t kT = 256;
constexpr uint32_t kHashLog = 14;
constexpr uint32_t kNoCand = 0xFFFFu;
constexpr uint32_t kMaxSeq = kUnit / kMinMatch;
constexpr uint32_t kQuarter = kUnit / 4;  // positions one wave parses
constexpr uint32_t kWords = kUnit / 4;     // bitstream words (the hash table's bytes)
constexpr uint32_t kUStride = kUnit + 16;  // a unit's slot: 3 header bytes + at most kUnit
static_assert((2u << kHashLog) == kUnit, "the hash table and the bitstream share 32 KiB");
static_assert(kUnit <= 32768, "positions, lengths and distances are kept in 16 bits");

struct ZTot {
  unsigned long long n_units, bound_bytes, data_bytes;
  // OKV_F_ZSTD_HUFFMAN: bit 0, a unit of the call wrote Huffman literals; bit 1
  // (OKV_F_ZSTD_HUF_FSE), one of them with FSE-compressed weights
  unsigned long long huf_seen;
};

__host__ __device__ inline uint64_t units_of(uint64_t orig) { return (orig + kUnit - 1) / kUnit; }
__host__ __device__ inline uint64_t padded(uint64_t len, uint64_t D) { return len + (D - len % D); }

// Exclusive scan of v[0..1024) in place by one thread; returns the total.
__device__ inline uint64_t serial_scan(uint64_t* v, uint32_t n) {
  uint64_t run = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t x = v[i];
    v[i] = run;
    run += x;
  }
  return run;
}

// Z1.  One workgroup; thread t owns a contiguous range of blocks.
__global__ __launch_bounds__(1024) void okv_zenc_plan_kernel(const Desc* __restrict__ img,
                                                             uint64_t nb, uint64_t D,
                                                             Desc* __restrict__ hdesc,
                                                             uint64_t* __restrict__ ubase,
                                                             ZTot* __restrict__ tot) {
  __shared__ uint64_t su[1024], sb[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t c = (nb + 1023) / 1024;
  const uint64_t k0 = min(nb, t * c), k1 = min(nb, k0 + c);
  uint64_t u = 0, by = 0;
  for (uint64_t k = k0; k < k1; ++k) {
    const uint64_t orig = img[k].original_size;
    u += units_of(orig);
    by += padded(frame_bound(orig), D);
  }
  su[t] = u, sb[t] = by;
  __syncthreads();
  if (t == 0) {
    tot->n_units = serial_scan(su, 1024);
    tot->bound_bytes = serial_scan(sb, 1024);
    ubase[nb] = tot->n_units;
  }
  __syncthreads();
  u = su[t];
  for (uint64_t k = k0; k < k1; ++k) {
    const Desc d = img[k];
    ubase[k] = u;
    hdesc[k] = Desc{d.offset, d.original_size, d.original_size, d.original_size};
    u += units_of(d.original_size);
  }
}

// The three predefined encode tables, built once per context (one lane per table) and
// copied into LDS by every unit.
__global__ void okv_zenc_tables_kernel(CTable* ct) {
  if (threadIdx.x < 3) build_ctable(ct[threadIdx.x], threadIdx.x);
}
static_assert(sizeof(CTable) % 4 == 0, "copied as words");

struct UnitSmem {
  uint4 src4[kUnit / 16 + 3];  // line 0 unused, the unit from line 1 (stage_block_wg)
  uint16_t cand[kUnit];
  uint32_t tab[kWords];
  uint8_t st[3][kMaxSeq];  // per sequence and chain: (1 << nb) | bits of its state step
  CTable ct[3];
  uint32_t s_bits[kT], s_lit[kT], s_ml[kT];
  uint32_t fin[3];
  uint32_t tot_bits, tot_lit;
  uint32_t blk, qcnt[4], qtail[4];
};

struct UnitParams {
  const uint8_t* img;
  const Desc* hdesc;      // offset into img, block_size = OriginalSize
  const uint64_t* ubase;  // [nb + 1]
  const CTable* ctabs;    // [3] okv_zenc_tables_kernel
  uint64_t nb;
  uint8_t* ubuf;    // [n_units][kUStride]
  uint32_t* usize;  // [n_units] bytes of the unit's zstd block, header included
};

__device__ __forceinline__ uint32_t load4(const uint32_t* w, uint32_t i) {
  return funnel(w[(i >> 2) + 1], w[i >> 2], i & 3);
}

__device__ __forceinline__ void or_bits(uint32_t* words, uint32_t pos, uint64_t v) {
  const uint32_t w = pos >> 5, sh = pos & 31;
  const uint64_t a = v << sh;
  const uint32_t a0 = uint32_t(a), a1 = uint32_t(a >> 32), a2 = sh ? uint32_t(v >> (64 - sh)) : 0;
  if (a0 && w < kWords) atomicOr(&words[w], a0);
  if (a1 && w + 1 < kWords) atomicOr(&words[w + 1], a1);
  if (a2 && w + 2 < kWords) atomicOr(&words[w + 2], a2);
}

// or_bits over `nw` words anywhere in LDS (the Huffman streams).
__device__ __forceinline__ void or_bits_n(uint32_t* words, uint32_t nw, uint32_t pos, uint64_t v) {
  const uint32_t w = pos >> 5, sh = pos & 31;
  const uint64_t a = v << sh;
  const uint32_t a0 = uint32_t(a), a1 = uint32_t(a >> 32), a2 = sh ? uint32_t(v >> (64 - sh)) : 0;
  if (a0 && w < nw) atomicOr(&words[w], a0);
  if (a1 && w + 1 < nw) atomicOr(&words[w + 1], a1);
  if (a2 && w + 2 < nw) atomicOr(&words[w + 2], a2);
}

// Where the Huffman phases (OKV_F_ZSTD_HUFFMAN) keep their tables: words of `tab`, which is
// dead between phase D and the point where H zeroes it.
constexpr uint32_t kHufHist = 0;     // [256] literal histogram
constexpr uint32_t kHufCode = 256;   // [kHufSyms, kHufAllSyms under kModeFse] (value << 4) | length
constexpr uint32_t kHufBits = 512;   // [kT] code bits of a thread's literals, then of the later ones
constexpr uint32_t kHufTot = 768;    // [0..3] code bits per stream, [4] longest code, [5] largest symbol,
                                     // [6] FSE description: its header bytes, then its bytes (0: none)
constexpr uint32_t kHufWorkAt = 1024;
constexpr uint32_t kWtAt = kHufWorkAt + kHufAllWork;  // WtWork (kModeFse)
static_assert(kHufWorkAt + kHufWork <= kWords && kHufSyms <= 256, "the Huffman tables fit tab");
static_assert(kHufCode + kHufAllSyms <= kHufBits && kHufBits + kT <= kHufTot &&
                  kHufTot + 7 <= kHufWorkAt && kWtAt + sizeof(WtWork) / 4 <= kWords,
              "the tables of all 256 symbols and the weights' description fit tab");
// What a unit's literals may become: raw only, Huffman with direct weights (OKV_F_ZSTD_HUFFMAN),
// or Huffman over all byte values with either description (OKV_F_ZSTD_HUF_FSE).
constexpr uint32_t kModeRaw = 0, kModeHuf = 1, kModeFse = 2;

// The unit's literals in order, by the whole workgroup: wave w takes the sequences of threads
// 64w .. 64w+63 (c sequences a thread, their literal and match lengths scanned in s_lit and
// s_ml), then all threads the tail behind the last sequence.  put(k, p): literal k of the
// unit's literals is byte p of the unit.
template <class Put>
__device__ __forceinline__ void each_literal(const uint16_t* sq, const uint32_t* s_lit,
                                             const uint32_t* s_ml, uint32_t ns, uint32_t c,
                                             uint32_t tot_lit, uint32_t lit_tail, uint32_t n,
                                             Put put) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, t0 = tid & ~63u;
  const uint32_t ka = min(ns, t0 * c), kb = min(ns, (t0 + 64) * c);
  uint32_t lp = s_lit[t0], sp = s_lit[t0] + s_ml[t0];
  for (uint32_t k = ka; k < kb; ++k) {
    const uint32_t ll = sq[3 * k], ml = sq[3 * k + 1];
    for (uint32_t j = lane; j < ll; j += 64) put(lp + j, sp + j);
    lp += ll;
    sp += ll + ml;
  }
  for (uint32_t j = tid; j < n - lit_tail; j += kT) put(tot_lit + j, lit_tail + j);
}

// Z2.  The phases, each ended by a barrier:
//  A  stage the unit (LDS DMA), copy the three encode tables, clear the hash table
//  B  hash of every 4-byte window
//  C  wave 0, 64 positions a step in order: each position gets the most recent earlier
//     position with its hash (equal hashes inside a step are resolved by ballot)
//  D  candidates whose 4 bytes differ are dropped
//  E  the greedy parse, one wave per quarter of the unit: a ballot over the next 64
//     positions finds the first with a candidate, the lanes extend its match 64 bytes a
//     step; then the four lists are made one
//  F  lanes 0-2: the three FSE state chains, last sequence to first
//  G  bit counts and literal counts per thread range, their scan, Compressed or Raw
//  H  every sequence's bits ORed into place; literals, headers and bitstream stored
// HUF (okv_zenc_unit_huf_kernel, OKV_F_ZSTD_HUFFMAN) adds between G and H, with the parse and
// the sequences unchanged:
//  L1 the literals gathered behind the sequences in `cand` (6 ns bytes of sequences, then at
//     most n - 4 ns literals; without a sequence they are the staged unit), their histogram
//     by LDS atomics
//  L2 one lane: code lengths and canonical codes (okv_zstd_enc.hpp); not eligible -> raw
//     kModeFse (okv_zenc_unit_fse_kernel): lengths over all 256 values, the listed weights,
//     their norm, NCount header and encode table by that lane; the two state chains on lanes
//     0 and 1; the description's bits packed by lane 0; FSE or direct by size
//  L3 every thread sums the code bits of its contiguous literals of one stream; one lane
//     per stream scans them; the section's size, Huffman or raw, Compressed or Raw
//  L4 the codes ORed into the stream words behind the gathered literals (they are fewer
//     bytes than the literals: 6 ns + 2 (n - 4 ns) <= 65 536), last literal first
//  L5 header, tree description (direct, or the compressed size and the FSE bytes), jump table
//     and streams stored
template <uint32_t MODE>
__device__ __forceinline__ void unit_body(const UnitParams& P, unsigned long long* huf_seen) {
  constexpr bool HUF = MODE != kModeRaw, FSE = MODE == kModeFse;
  __shared__ UnitSmem sm;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t u = blockIdx.x;
  if (tid == 0) {  // the block this unit belongs to: last b with ubase[b] <= u
    uint64_t lo = 0, hi = P.nb;
    while (hi - lo > 1) {
      const uint64_t m = (lo + hi) / 2;
      if (P.ubase[m] <= u) lo = m; else hi = m;
    }
    sm.blk = uint32_t(lo);
  }
  for (uint32_t i = tid; i < 3 * sizeof(CTable) / 4; i += kT)
    reinterpret_cast<uint32_t*>(sm.ct)[i] = reinterpret_cast<const uint32_t*>(P.ctabs)[i];
  for (uint32_t i = tid; i < kWords; i += kT) sm.tab[i] = 0xFFFFFFFFu;
  __syncthreads();
  const uint64_t b = sm.blk;
  const Desc hd = P.hdesc[b];
  const uint64_t ku = u - P.ubase[b];
  const uint64_t left = hd.block_size - ku * kUnit;
  const uint32_t n = uint32_t(left < kUnit ? left : kUnit);
  const bool last = left <= kUnit;
  stage_block_wg<kT>(sm.src4, P.img, hd.offset + ku * kUnit, n);
  __syncthreads();
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(sm.src4 + 1);
  const uint8_t* sb = reinterpret_cast<const uint8_t*>(sm.src4 + 1);
  uint16_t* tab16 = reinterpret_cast<uint16_t*>(sm.tab);
  const uint32_t npos = n >= kMinMatch ? n - (kMinMatch - 1) : 0;  // positions with a window
  // B
  for (uint32_t i = tid; i < npos; i += kT)
    sm.cand[i] = uint16_t((load4(sw, i) * 2654435761u) >> (32 - kHashLog));
  __syncthreads();
  // C
  if (wave == 0) {
    volatile uint16_t* tb = tab16;
    for (uint32_t base = 0; base < npos; base += 64) {
      const uint32_t i = base + lane;
      const bool act = i < npos;
      const uint32_t h = act ? sm.cand[i] : 0;
      uint32_t c = act ? tb[h] : kNoCand;  // the most recent position of an earlier step
      if (act) tb[h] = uint16_t(i);
      const uint32_t w = act ? tb[h] : i;
      uint64_t conf = __ballot(act && w != i);  // lanes that share a hash with another lane
      while (conf) {
        const int f = __ffsll((long long)conf) - 1;
        const uint32_t h0 = uint32_t(__builtin_amdgcn_readlane(int(h), f));
        const bool mine = act && h == h0;
        const uint64_t grp = __ballot(mine);
        if (mine) {
          const uint64_t lower = grp & ((uint64_t(1) << lane) - 1);
          if (lower) c = base + 63 - __clzll((long long)lower);
          if ((grp >> lane) == 1) tb[h0] = uint16_t(i);  // the group's last lane stays
        }
        conf &= ~grp;
      }
      if (act) sm.cand[i] = uint16_t(c);
    }
  }
  __syncthreads();
  // D
  for (uint32_t i = tid; i < npos; i += kT) {
    const uint32_t c = sm.cand[i];
    if (c != kNoCand && load4(sw, c) != load4(sw, i)) sm.cand[i] = uint16_t(kNoCand);
  }
  __syncthreads();
  // E: wave q parses the quarter [q * kQuarter, (q + 1) * kQuarter) of the unit; a match may
  // start and end only inside its quarter (its source is anywhere before it).  The wave's
  // sequence k goes to cand[q * kQuarter + 3k ..]: its parse is past position 4(k+1) of the
  // quarter by then, and 3 * (kQuarter / 4) entries stay inside the quarter.
  uint16_t* sq = sm.cand;
  {
    const uint32_t q0 = min(wave * kQuarter, n), qe = min(q0 + kQuarter, n);
    const uint32_t pe = min(npos, qe >= kMinMatch ? qe - (kMinMatch - 1) : 0u);  // match starts
    uint16_t* wq = sq + wave * kQuarter;
    uint32_t p = q0, lit0 = q0, ns = 0;
    while (p < pe) {
      const uint32_t i = p + lane;
      const uint32_t c = i < pe ? sm.cand[i] : kNoCand;
      const uint64_t m = __ballot(c != kNoCand);
      if (!m) {
        p += 64;
        continue;
      }
      const int f = __ffsll((long long)m) - 1;
      const uint32_t s = p + f, cs = uint32_t(__builtin_amdgcn_readlane(int(c), f));
      uint32_t len = kMinMatch;
      for (;;) {
        const uint32_t j = len + lane;
        const bool ne = s + j >= qe || sb[s + j] != sb[cs + j];
        const uint64_t mm = __ballot(ne);
        if (mm) {
          len += __ffsll((long long)mm) - 1;
          break;
        }
        len += 64;
      }
      if (lane == 0) {
        wq[3 * ns] = uint16_t(s - lit0);
        wq[3 * ns + 1] = uint16_t(len);
        wq[3 * ns + 2] = uint16_t(s - cs);
      }
      ++ns;
      p = lit0 = s + len;
    }
    if (lane == 0) sm.qcnt[wave] = ns, sm.qtail[wave] = lit0;
  }
  __syncthreads();
  // the quarters' sequences made one list at cand[0 ..]: moved down 256 entries a step
  // (read, barrier, write: a step's destination lies below every later step's source);
  // literals left at a quarter's end join the next sequence's literal length
  uint32_t ns = 0, lit_tail = 0;
  {
    uint32_t carry = 0;
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t q0 = min(q * kQuarter, n), qe = min(q0 + kQuarter, n);
      const uint32_t cnt = sm.qcnt[q];
      if (!cnt) {
        carry += qe - q0;
        continue;
      }
      const uint32_t src = q * kQuarter, dst = 3 * ns, len = 3 * cnt;
      if (src != dst || carry) {
        for (uint32_t j0 = 0; j0 < len; j0 += kT) {
          const uint32_t j = j0 + tid;
          uint32_t v = j < len ? sq[src + j] : 0;
          if (j == 0) v += carry;
          __syncthreads();
          if (j < len) sq[dst + j] = uint16_t(v);
        }
      }
      ns += cnt;
      carry = qe - sm.qtail[q];
    }
    lit_tail = n - carry;
  }
  __syncthreads();
  uint8_t* out = P.ubuf + u * kUStride;
  bool comp = ns > 0;
  uint32_t csz = 0, nlit = 0, own_bits = 0;
  const uint32_t c = (ns + kT - 1) / kT;
  const uint32_t k0 = min(ns, tid * c), k1 = min(ns, k0 + c);
  if (comp) {
    // F: the symbols by all threads, so that a chain step waits for one look-up only
    for (uint32_t k = tid; k < ns; k += kT) {
      const SeqCode sc = seq_code(sq[3 * k], sq[3 * k + 1], sq[3 * k + 2]);
      for (uint32_t t = 0; t < 3; ++t) sm.st[t][k] = uint8_t(sc.sym[t]);
    }
    __syncthreads();
    if (tid < 3) {
      const CTable& ct = sm.ct[tid];
      uint8_t* st = sm.st[tid];
      uint32_t k = ns - 1;
      uint32_t state = fse_init(ct, st[k]);
      st[k] = 1;
#pragma unroll 4
      while (k-- > 0) {
        uint32_t nb, bits;
        state = fse_step(ct, state, st[k], nb, bits);
        st[k] = uint8_t((1u << nb) | bits);
      }
      sm.fin[tid] = state;
    }
    __syncthreads();
    // G
    uint32_t own_lit = 0, own_ml = 0;
    for (uint32_t k = k0; k < k1; ++k) {
      const uint32_t ll = sq[3 * k], ml = sq[3 * k + 1], off = sq[3 * k + 2];
      const SeqCode sc = seq_code(ll, ml, off);
      own_bits += sc.xb[kLL] + sc.xb[kML] + sc.xb[kOF] + highbit(sm.st[0][k]) +
                  highbit(sm.st[1][k]) + highbit(sm.st[2][k]);
      own_lit += ll;
      own_ml += ml;
    }
    sm.s_bits[tid] = own_bits, sm.s_lit[tid] = own_lit, sm.s_ml[tid] = own_ml;
    __syncthreads();
    if (tid < 3) {  // one lane per array: the exclusive scan in place
      uint32_t* a = tid == 0 ? sm.s_bits : tid == 1 ? sm.s_lit : sm.s_ml;
      uint32_t run = 0;
      for (uint32_t i = 0; i < kT; ++i) {
        const uint32_t x = a[i];
        a[i] = run;
        run += x;
      }
      if (tid == 0) sm.tot_bits = run;
      if (tid == 1) sm.tot_lit = run;
    }
    __syncthreads();
    nlit = sm.tot_lit + (n - lit_tail);
    if constexpr (!HUF) {
      csz = compressed_size(nlit, ns, uint64_t(sm.tot_bits) + 18);
      comp = csz < n;
    }
  }
  // the Huffman phases: `huf` says the literals section is a Compressed_Literals_Block of
  // `litsec` bytes whose streams take hb0 .. hb3 bytes
  bool huf = false, dfse = false;
  uint32_t litsec = 0, hmb = 0, hlast = 0, hsum = 0, hlo = 0, hhi = 0, hstream = 0, hdesc = 0;
  uint32_t hb0 = 0, hb1 = 0, hb2 = 0, hb3 = 0;
  const auto streams_before = [&](uint32_t s) {  // bytes of the streams before stream s
    return (s > 0 ? hb0 : 0) + (s > 1 ? hb1 : 0) + (s > 2 ? hb2 : 0);
  };
  uint8_t* cb = reinterpret_cast<uint8_t*>(sm.cand);
  const uint8_t* lits = sb;
  if constexpr (HUF) {
    uint32_t* hist = sm.tab + kHufHist;
    uint32_t* code = sm.tab + kHufCode;
    uint32_t* tbits = sm.tab + kHufBits;
    uint32_t* htot = sm.tab + kHufTot;
    // L1
    hist[tid] = 0;
    __syncthreads();
    if (ns) {
      uint8_t* lb = cb + 6 * ns;
      each_literal(sq, sm.s_lit, sm.s_ml, ns, c, sm.tot_lit, lit_tail, n,
                   [&](uint32_t k, uint32_t p) {
                     const uint32_t v = sb[p];
                     lb[k] = uint8_t(v);
                     atomicAdd(&hist[v], 1u);
                   });
      lits = lb;
    } else {
      nlit = n;
      for (uint32_t j = tid; j < n; j += kT) atomicAdd(&hist[sb[j]], 1u);
    }
    __syncthreads();
    // L2
    WtWork& wt = *reinterpret_cast<WtWork*>(sm.tab + kWtAt);
    if (tid == 0) {
      if constexpr (FSE) {
        const uint32_t mb = huf_lengths_all(hist, code, sm.tab + kHufWorkAt);
        const uint32_t lastsym = mb ? huf_codes_all(code, mb, code, sm.tab + kHufWorkAt) : 0;
        for (uint32_t s = 0; s < lastsym; ++s) wt.w[s] = uint8_t(huf_weight(code[s] & 15u, mb));
        htot[4] = mb, htot[5] = lastsym;
        htot[6] = mb ? wt_prepare(wt, lastsym) : 0;
      } else {
        const uint32_t mb = huf_lengths(hist, code, sm.tab + kHufWorkAt);
        htot[4] = mb;
        htot[5] = mb ? huf_codes(code, mb, code, sm.tab + kHufWorkAt) : 0;
      }
    }
    __syncthreads();
    hmb = htot[4], hlast = htot[5];
    if constexpr (FSE) {
      const uint32_t nc = htot[6];  // (the same for every thread)
      if (nc) {
        if (tid < 2) wt_chain(wt, hlast, tid);
        __syncthreads();
        if (tid == 0) htot[6] = wt_pack(wt, hlast, nc);
        __syncthreads();
      }
      hdesc = huf_desc_size(hlast, htot[6], dfse);
      if (!hdesc) hmb = 0;  // a value above kHufMaxSym and no FSE description: raw
    } else {
      hdesc = huf_tree_size(hlast);
    }
    litsec = lit_header_size(nlit) + nlit;
    if (hmb) {
      // L3: 256 threads on the one stream, or 64 on each of four
      const uint32_t nstr = huf_streams(nlit), tps = kT / nstr;
      hstream = tid / tps;
      const uint32_t j = tid % tps, cnt = huf_stream_len(nlit, hstream);
      const uint32_t first = hstream * huf_stream_len(nlit, 0), ch = (cnt + tps - 1) / tps;
      hlo = first + min(cnt, j * ch), hhi = first + min(cnt, j * ch + ch);
      uint32_t own = 0;
      for (uint32_t i = hlo; i < hhi; ++i) own += code[lits[i]] & 15u;
      tbits[tid] = own;
      __syncthreads();
      if (tid < nstr) {  // one lane per stream: the bits of the later literals, in place
        uint32_t run = 0;
        for (uint32_t k = tps; k-- > 0;) {
          const uint32_t x = tbits[tid * tps + k];
          tbits[tid * tps + k] = run;
          run += x;
        }
        htot[tid] = run;
      }
      __syncthreads();
      hb0 = huf_stream_bytes(htot[0]);
      if (nstr == 4)
        hb1 = huf_stream_bytes(htot[1]), hb2 = huf_stream_bytes(htot[2]),
        hb3 = huf_stream_bytes(htot[3]);
      hsum = hb0 + hb1 + hb2 + hb3;
      if constexpr (FSE) {
        huf = huf_wins_d(nlit, hdesc, hsum);
        if (huf) litsec = huf_section_size_d(nlit, hdesc, hsum);
      } else {
        huf = huf_wins(nlit, hlast, hsum);
        if (huf) litsec = huf_section_size(nlit, hlast, hsum);
      }
    }
    // every thread has read what decides its way from here (htot); only now may a thread
    // that goes straight to H, or to the Raw_Block, write into tab
    __syncthreads();
    csz = block_content_size(litsec, ns, ns ? uint64_t(sm.tot_bits) + 18 : 0);
    comp = csz < n;
  }
  if (!comp) {  // Raw_Block
    if (tid == 0) {
      block_header(out, last, kBlockRaw, n);
      P.usize[u] = 3 + n;
    }
    for (uint32_t j = tid; j < n; j += kT) out[3 + j] = sb[j];
    return;
  }
  if constexpr (HUF) {
    if (huf) {
      // L4: the stream words lie behind the literals (behind nothing without a sequence:
      // the literals are then the staged unit)
      const uint32_t hoff = ns ? (6 * ns + nlit + 3) & ~3u : 0;
      uint32_t* hw = reinterpret_cast<uint32_t*>(cb + hoff);
      const uint32_t nw = min((hsum + 3) / 4, (2 * kUnit - hoff) / 4);
      const uint32_t* code = sm.tab + kHufCode;
      for (uint32_t i = tid; i < nw; i += kT) hw[i] = 0;
      __syncthreads();
      uint32_t pos = 8 * streams_before(hstream) + sm.tab[kHufBits + tid], an = 0;
      uint64_t acc = 0;
      for (uint32_t i = hhi; i-- > hlo;) {
        const uint32_t cd = code[lits[i]];
        acc |= uint64_t(cd >> 4) << an;
        an += cd & 15u;
        if (an > 64 - kHufMaxBits) {
          or_bits_n(hw, nw, pos, acc);
          pos += an;
          acc = 0, an = 0;
        }
      }
      if (an) or_bits_n(hw, nw, pos, acc);
      if (tid < huf_streams(nlit))  // the end mark of stream `tid`, above its last code
        or_bits_n(hw, nw, 8 * streams_before(tid) + sm.tab[kHufTot + tid], 1);
      __syncthreads();
      // L5
      const uint32_t hh = huf_header_size(nlit), ts = hdesc;
      const uint32_t jt = huf_streams(nlit) == 4 ? 6 : 0;
      uint8_t* sec = out + 3;
      if (tid == 0) {
        huf_header(sec, nlit, ts + jt + hsum);
        atomicOr(huf_seen, dfse ? 3ull : 1ull);
      }
      if (FSE && dfse) {
        const uint8_t* fo = reinterpret_cast<const WtWork*>(sm.tab + kWtAt)->out;
        for (uint32_t k = tid; k < ts; k += kT) sec[hh + k] = k ? fo[k - 1] : uint8_t(ts - 1);
      } else {
        for (uint32_t k = tid; k < ts; k += kT) sec[hh + k] = huf_tree_byte(code, hmb, hlast, k);
      }
      if (jt && tid < 3) {
        const uint32_t by = tid == 0 ? hb0 : tid == 1 ? hb1 : hb2;
        sec[hh + ts + 2 * tid] = uint8_t(by);
        sec[hh + ts + 2 * tid + 1] = uint8_t(by >> 8);
      }
      for (uint32_t j = tid; j < hsum; j += kT)
        sec[hh + ts + jt + j] = uint8_t(hw[j >> 2] >> (8 * (j & 3)));
      __syncthreads();  // the code table is read; H takes tab
    }
    if (!ns) {  // literals only: the sequences section is the byte 0
      if (tid == 0) {
        block_header(out, last, kBlockCompressed, csz);
        out[3 + litsec] = 0;
        P.usize[u] = 3 + csz;
      }
      return;
    }
  }
  // H
  const uint32_t tot_bits = sm.tot_bits;
  const uint32_t nwords = min(kWords, (tot_bits + 18 + 31) / 32 + 1);
  for (uint32_t i = tid; i < nwords; i += kT) sm.tab[i] = 0;
  __syncthreads();
  {
    uint32_t pos = tot_bits - sm.s_bits[tid] - own_bits;  // bits of every later sequence
    for (uint32_t k = k1; k-- > k0;) {
      const SeqCode sc = seq_code(sq[3 * k], sq[3 * k + 1], sq[3 * k + 2]);
      uint32_t nb[3], bits[3];
      for (uint32_t t = 0; t < 3; ++t) {
        const uint32_t e = sm.st[t][k];
        nb[t] = highbit(e);
        bits[t] = e - (1u << nb[t]);
      }
      const SeqBits sbits = seq_bits(sc, nb, bits);  // (at most 60 bits at this unit size)
      or_bits(sm.tab, pos, sbits.lo);
      pos += sbits.nb;
    }
    if (tid == 0) or_bits(sm.tab, tot_bits, close_bits(sm.fin).lo);
  }
  const uint32_t lh = lit_header_size(nlit);
  uint8_t* lit_out = out + 3 + lh;
  if (!HUF || !huf)
    each_literal(sq, sm.s_lit, sm.s_ml, ns, c, sm.tot_lit, lit_tail, n,
                 [&](uint32_t k, uint32_t p) { lit_out[k] = sb[p]; });
  __syncthreads();  // the bitstream words are complete
  uint8_t* seq_out = HUF ? out + 3 + litsec : lit_out + nlit;
  const uint32_t sh = nseq_header_size(ns);
  if (tid == 0) {
    block_header(out, last, kBlockCompressed, csz);
    if (!HUF || !huf) lit_header(out + 3, nlit);
    nseq_header(seq_out, ns);
    seq_out[sh] = 0;  // Predefined_Mode x 3
    P.usize[u] = 3 + csz;
  }
  const uint32_t nbytes = (tot_bits + 18 + 7) >> 3;
  for (uint32_t j = tid; j < nbytes; j += kT)
    seq_out[sh + 1 + j] = uint8_t(sm.tab[j >> 2] >> (8 * (j & 3)));
}

__global__ __launch_bounds__(kT) void okv_zenc_unit_kernel(UnitParams P) {
  unit_body<kModeRaw>(P, nullptr);
}
// The same unit with Huffman-coded literals where they are smaller; *huf_seen becomes 1 when
// a unit of the launch wrote a Compressed_Literals_Block.
__global__ __launch_bounds__(kT) void okv_zenc_unit_huf_kernel(UnitParams P,
                                                               unsigned long long* huf_seen) {
  unit_body<kModeHuf>(P, huf_seen);
}
// The same over all 256 byte values, the tree described by direct or by FSE-compressed weights,
// whichever is smaller (OKV_F_ZSTD_HUF_FSE); *huf_seen gains bit 1 when a unit wrote the latter.
__global__ __launch_bounds__(kT) void okv_zenc_unit_fse_kernel(UnitParams P,
                                                               unsigned long long* huf_seen) {
  unit_body<kModeFse>(P, huf_seen);
}

// Z4.  One workgroup; thread t owns a contiguous range of blocks.
__global__ __launch_bounds__(1024) void okv_zenc_size_kernel(
    const Desc* __restrict__ hdesc, const uint64_t* __restrict__ ubase,
    const uint32_t* __restrict__ usize, uint64_t nb, uint64_t D, Desc* __restrict__ desc,
    uint64_t* __restrict__ uoff, ZTot* __restrict__ tot) {
  __shared__ uint64_t sb[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t c = (nb + 1023) / 1024;
  const uint64_t k0 = min(nb, t * c), k1 = min(nb, k0 + c);
  uint64_t by = 0;
  for (uint64_t k = k0; k < k1; ++k) {
    const uint64_t orig = hdesc[k].original_size;
    uint64_t pos = frame_header_size(orig);
    for (uint64_t u = ubase[k]; u < ubase[k + 1]; ++u) {
      uoff[u] = pos;
      pos += usize[u];
    }
    const uint64_t cs = pos + 4;  // Content_Checksum
    const uint64_t bs = padded(cs, D);
    desc[k] = Desc{0, bs, orig, cs};
    by += bs;
  }
  sb[t] = by;
  __syncthreads();
  if (t == 0) tot->data_bytes = serial_scan(sb, 1024);
  __syncthreads();
  uint64_t run = sb[t];
  for (uint64_t k = k0; k < k1; ++k) {
    desc[k].offset = run;
    run += desc[k].block_size;
  }
}

struct PlaceParams {
  const Desc* desc;
  const uint64_t* ubase;
  const uint64_t* uoff;
  const uint32_t* usize;
  const uint8_t* ubuf;
  const uint64_t* raw_hash;  // XXH64 of each raw block
  uint8_t* seg;
  int aligned;  // block offsets and seg are 16-byte aligned
};

// Z5.  One workgroup per block; a thread assembles 16 destination bytes and stores them
// once: frame header, the units' zstd blocks, the checksum, then the zero padding.
__global__ __launch_bounds__(kT) void okv_zenc_place_kernel(PlaceParams P) {
  __shared__ uint8_t hdr[16], ck[4];
  const uint64_t b = blockIdx.x;
  const Desc d = P.desc[b];
  const uint64_t u0 = P.ubase[b], nu = P.ubase[b + 1] - u0;
  const uint64_t hs = frame_header_size(d.original_size), cs = d.compressed_size;
  if (threadIdx.x == 0) {
    frame_header(hdr, d.original_size);
    const uint32_t x = uint32_t(P.raw_hash[b]);
    for (int i = 0; i < 4; ++i) ck[i] = uint8_t(x >> (8 * i));
  }
  __syncthreads();
  uint8_t* dst = P.seg + d.offset;
  const uint64_t nq = (d.block_size + 15) / 16;
  for (uint64_t q = threadIdx.x; q < nq; q += kT) {
    const uint64_t f0 = 16 * q;
    uint32_t w[4] = {0, 0, 0, 0};
    if (f0 < cs) {
      uint64_t cu_beg = 0, cu_end = 0, cu = 0;
      for (uint32_t j = 0; j < 16; ++j) {
        const uint64_t f = f0 + j;
        if (f >= cs) break;
        uint32_t v;
        if (f < hs) {
          v = hdr[f];
        } else if (f < cs - 4) {
          if (f >= cu_end) {  // the unit holding frame byte f: last u with uoff[u] <= f
            uint64_t lo = 0, hi = nu;
            while (hi - lo > 1) {
              const uint64_t m = (lo + hi) / 2;
              if (P.uoff[u0 + m] <= f) lo = m; else hi = m;
            }
            cu = u0 + lo;
            cu_beg = P.uoff[cu];
            cu_end = cu_beg + P.usize[cu];
          }
          v = P.ubuf[cu * kUStride + (f - cu_beg)];
        } else {
          v = ck[f - (cs - 4)];
        }
        w[j >> 2] |= v << (8 * (j & 3));
      }
    }
    if (P.aligned) {
      *reinterpret_cast<uint4*>(dst + f0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (uint32_t j = 0; j < 16 && f0 + j < d.block_size; ++j)
        dst[f0 + j] = uint8_t(w[j >> 2] >> (8 * (j & 3)));
    }
  }
}

// The stage's scratch: owned here, reached from okv_ctx through one pointer, released by
// okv_close (zstd_enc_release).
struct Scratch {
  DevBuf<Desc> hdesc;         // [nb] raw block: offset into the image, BlockSize = OriginalSize
  DevBuf<uint64_t> ubase;     // [nb + 1] units before each block
  DevBuf<uint32_t> usize;     // [n_units]
  DevBuf<uint64_t> uoff;      // [n_units] place of the unit inside its frame
  DevBuf<uint8_t> ubuf;       // [n_units][kUStride]
  DevBuf<uint64_t> raw_hash;  // [nb]
  DevBuf<CTable> ctabs;       // [3] the predefined encode tables (built once)
  DevBuf<ZTot> d_tot;
  PinBuf<ZTot> h_tot;
  uint64_t nb = 0;            // of the last zstd_enc_bound
};

int read_tot(okv_ctx* ctx, Scratch* s) {
  OKV_HIP(hipMemcpyAsync(s->h_tot.data(), s->d_tot.data(), sizeof(ZTot), hipMemcpyDeviceToHost,
                         ctx->stream));
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  return OKV_OK;
}

}  // namespace zenc

int zstd_enc_bound(okv_ctx* ctx, const Desc* img_desc, uint64_t nb, uint64_t D,
                   uint64_t* bound_bytes) {
  if (!ctx->zenc) ctx->zenc = new zenc::Scratch();
  zenc::Scratch* s = ctx->zenc;
  int rc;
  if ((rc = reserve(ctx, s->d_tot, 1)) || (rc = reserve(ctx, s->h_tot, 1)) ||
      (rc = reserve(ctx, s->hdesc, nb)) || (rc = reserve(ctx, s->ubase, nb + 1)) ||
      (rc = reserve(ctx, s->raw_hash, nb)))
    return rc;
  hipLaunchKernelGGL(zenc::okv_zenc_plan_kernel, dim3(1), dim3(1024), 0, ctx->stream, img_desc, nb,
                     D, s->hdesc.data(), s->ubase.data(), s->d_tot.data());
  OKV_HIP(hipGetLastError());
  if ((rc = zenc::read_tot(ctx, s))) return rc;
  s->nb = nb;
  *bound_bytes = s->h_tot->bound_bytes;
  return OKV_OK;
}

int zstd_enc_run(okv_ctx* ctx, const uint8_t* img, uint64_t img_bytes, Desc* desc, uint64_t nb,
                 uint64_t D, uint8_t* seg, uint64_t* hash, uint64_t* data_bytes, uint32_t mode,
                 uint32_t* huffman_seen) {
  zenc::Scratch* s = ctx->zenc;
  if (!s || s->nb != nb || nb >= (uint64_t(1) << 32))
    return set_err(ctx, OKV_E_ARG, "zstd encode: no plan for these blocks");
  const uint64_t nu = s->h_tot->n_units;
  if (nu == 0 || nu >= (uint64_t(1) << 31))
    return set_err(ctx, OKV_E_ARG, "zstd encode: too many units for one call");
  int rc;
  if ((rc = reserve(ctx, s->usize, nu)) || (rc = reserve(ctx, s->uoff, nu)) ||
      (rc = reserve(ctx, s->ubuf, nu * zenc::kUStride)))
    return rc;
  bool fresh = false;
  if ((rc = reserve(ctx, s->ctabs, 3, &fresh))) return rc;
  if (fresh)
    hipLaunchKernelGGL(zenc::okv_zenc_tables_kernel, dim3(1), dim3(64), 0, ctx->stream,
                       s->ctabs.data());
  zenc::UnitParams up;
  up.img = img;
  up.ctabs = s->ctabs.data();
  up.hdesc = s->hdesc.data();
  up.ubase = s->ubase.data();
  up.nb = nb;
  up.ubuf = s->ubuf.data();
  up.usize = s->usize.data();
  // ZTot::huf_seen comes back with the sizes' read-back
  unsigned long long* huf_seen = &s->d_tot.data()->huf_seen;
  if (mode == kZencFse) {
    OKV_HIP(hipMemsetAsync(huf_seen, 0, sizeof *huf_seen, ctx->stream));
    hipLaunchKernelGGL(zenc::okv_zenc_unit_fse_kernel, dim3(uint32_t(nu)), dim3(zenc::kT), 0,
                       ctx->stream, up, huf_seen);
  } else if (mode == kZencHuffman) {
    OKV_HIP(hipMemsetAsync(huf_seen, 0, sizeof *huf_seen, ctx->stream));
    hipLaunchKernelGGL(zenc::okv_zenc_unit_huf_kernel, dim3(uint32_t(nu)), dim3(zenc::kT), 0,
                       ctx->stream, up, huf_seen);
  } else {
    hipLaunchKernelGGL(zenc::okv_zenc_unit_kernel, dim3(uint32_t(nu)), dim3(zenc::kT), 0,
                       ctx->stream, up);
  }
  launch_hash(ctx->stream, img, img_bytes, s->hdesc.data(), uint32_t(nb), s->raw_hash.data());
  hipLaunchKernelGGL(zenc::okv_zenc_size_kernel, dim3(1), dim3(1024), 0, ctx->stream,
                     s->hdesc.data(), s->ubase.data(), s->usize.data(), nb, D, desc,
                     s->uoff.data(), s->d_tot.data());
  OKV_HIP(hipGetLastError());
  if ((rc = zenc::read_tot(ctx, s))) return rc;
  *data_bytes = s->h_tot->data_bytes;
  *huffman_seen = mode == kZencRaw ? 0 : uint32_t(s->h_tot->huf_seen);
  if (*data_bytes > s->h_tot->bound_bytes)
    return set_err(ctx, OKV_E_HIP, "zstd encode: frames larger than their bound");
  zenc::PlaceParams pp;
  pp.desc = desc;
  pp.ubase = s->ubase.data();
  pp.uoff = s->uoff.data();
  pp.usize = s->usize.data();
  pp.ubuf = s->ubuf.data();
  pp.raw_hash = s->raw_hash.data();
  pp.seg = seg;
  pp.aligned = D % 16 == 0 && (reinterpret_cast<uintptr_t>(seg) & 15) == 0;
  hipLaunchKernelGGL(zenc::okv_zenc_place_kernel, dim3(uint32_t(nb)), dim3(zenc::kT), 0,
                     ctx->stream, pp);
  launch_hash(ctx->stream, seg, *data_bytes, desc, uint32_t(nb), hash);
  OKV_HIP(hipGetLastError());
  return OKV_OK;
}

void zstd_enc_release(okv_ctx* ctx) {
  delete ctx->zenc;  // the buffers release themselves
  ctx->zenc = nullptr;
}

}  // namespace okv
