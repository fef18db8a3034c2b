// okv_get_kernels.hpp -- the device pieces the batched GetRow of one segment
// (okv_get.hip) and of a snapshot (okv_snap.hip) are both made of: the three-launch
// exclusive scan, the grouping of items by block, the search of a staged block and the
// copy of a value; and the host steps both entry points share: the grouping and search
// launches, the totals, and the values tail of device and host mode (the end of this
// file).  Under OKV_F_GET_ZSTD the touched blocks of zstd segments are packed, inflated by
// the zstd stage and searched from its scratch (the "inflate arms").  An "item" is what lands on a block: a key (okv_get.hip) or a
// (key, segment) pair (okv_snap.hip).  Internal header of those two files; everything
// has internal linkage, so each file's code object holds its own kernels.
#pragma once
#include "okv_ctx.hpp"

#include "okv_bloom_hash.hpp"
#include "okv_index.hpp"
#include "okv_stage.hpp"

struct okv_index {
  okv_ctx* ctx = nullptr;
  uint64_t nt = 0, nf = 0;     // tree entries, entries given
  uint64_t max_block = 0;      // largest BlockSize in the tree
  uint64_t max_original = 0;   // largest OriginalSize in the tree
  uint32_t n_cu = 0;
  okv::DevBuf<okv::Desc> descs;        // [nt] tree order
  okv::DevBuf<uint32_t> file_index;    // [nt]
  okv::DevBuf<uint8_t> arena;          // first keys
  okv::DevBuf<uint64_t> off;           // [nt]
  okv::DevBuf<uint16_t> len;           // [nt]
  okv::DevBuf<uint64_t> prefix;        // [nt]
};

namespace okv {
namespace get {
namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kSmallCap = 8192;       // the search kernel's small stage (4 KiB blocks)
constexpr uint32_t kSearchThreads = 1024;  // 16 waves share a staged block's keys
constexpr uint32_t kScanPer = 8;           // elements per thread of a scan tile
constexpr uint32_t kScanTile = kThreads * kScanPer;
constexpr uint64_t kMaxK = 4096;           // as okv_bloom.hip

uint32_t ceil_div(uint64_t a, uint64_t b) { return uint32_t((a + b - 1) / b); }

// ---- locate: SegmentReader.GetRow up to the block read, for one key of one segment ----
struct Filter {  // a segment's bloom filter (k == 0: none, no probe)
  const uint64_t* words;
  bloom::Modulus mod;
  uint32_t k;
  uint64_t length;
};

// state / bst / entry as okv_get_out documents them; t is the floor block's tree position
// when the search takes the block (it is in the segment and: uncompressed or LZ4, at most
// kStage bytes; or zstd under OKV_F_GET_ZSTD (zget), whatever its BlockSize), else kNone.
__device__ __forceinline__ void locate_key(const uint8_t* key, uint32_t kl, const Filter& f,
                                           const index::View& ix, const Desc* descs,
                                           const uint32_t* file_index, uint64_t seg_bytes, int comp,
                                           bool zget, int32_t& state, int32_t& bst,
                                           uint32_t& entry, uint32_t& t) {
  state = OKV_GET_NOT_IN_BLOCK, bst = OKV_BLK_OK;
  entry = kNone, t = kNone;
  bool maybe = true;
  if (f.k) {  // Test (:371-378): a location >= length reads as unset (bitset.Test)
    uint64_t h[4];
    bloom::base_hashes(key, kl, h);
    for (uint32_t j = 0; j < f.k; ++j) {
      const uint64_t loc = bloom::location(h, j, f.mod);
      if (loc >= f.length || !((f.words[loc >> 6] >> (loc & 63)) & 1)) {
        maybe = false;
        break;
      }
    }
  }
  if (!maybe) {
    state = OKV_GET_BLOOM_NEGATIVE;
    return;
  }
  const uint64_t up = index::floor_upper(ix, key, kl, index::prefix8(key, kl));
  if (up == 0) {
    state = OKV_GET_NO_BLOCK;  // :387-389
    return;
  }
  const uint32_t tt = uint32_t(up - 1);
  const Desc d = descs[tt];
  entry = file_index[tt];
  const bool zstd = comp == OKV_COMP_ZSTD;
  bst = go_read_status(d, seg_bytes);  // :303-316, before any read
  // rawBlockBytes[:CompressedSize] (:321), as the zstd stage's zstd_raw_status has it
  if (bst == OKV_BLK_OK && zstd && zget && d.compressed_size > d.block_size) bst = OKV_BLK_PANIC;
  if (bst != OKV_BLK_OK)
    state = OKV_GET_BLOCK_ERROR;
  else if (zstd ? !zget : d.block_size > uint64_t(kStage))
    state = OKV_GET_FALLBACK;
  else
    t = tt;
}

// ---- exclusive scan of a u64 per element: tile sums (wg_excl_scan, okv_kernels.hpp), their
// scan by the encode's one-workgroup kernel (launch_scan_u64), the tiles again.  Three
// launches; no workgroup waits for another. -------------------------------------------
struct CntLoad {  // items on the block | (block touched) << 32
  const uint32_t* cnt;
  __device__ uint64_t operator()(uint64_t i) const {
    const uint32_t c = cnt[i];
    return uint64_t(c) | (uint64_t(c != 0) << 32);
  }
};
struct ValLoad {  // arena room of the key's value (state 0: OKV_GET_FOUND, OKV_SNAP_FOUND)
  const int32_t* state;
  const uint32_t* val_len;
  __device__ uint64_t operator()(uint64_t i) const {
    return state[i] == OKV_GET_FOUND ? round16(val_len[i]) : 0;
  }
};

template <class Load>
__global__ __launch_bounds__(kThreads) void okv_get_scan_sums_kernel(Load ld, uint64_t n,
                                                                     uint64_t* __restrict__ tsum) {
  __shared__ uint64_t sm[kThreads / 64 + 1];
  const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanPer;
  uint64_t s = 0;
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j)
    if (base + j < n) s += ld(base + j);
  uint64_t total;
  (void)wg_excl_scan(s, sm, total);
  if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// out[i] = sum of ld(j), j < i; out[n] = the total; out2 (may be null): out[0 .. n) again
template <class Load>
__global__ __launch_bounds__(kThreads) void okv_get_scan_write_kernel(
    Load ld, uint64_t n, const uint64_t* __restrict__ tsum, uint64_t* __restrict__ out,
    uint64_t* __restrict__ out2) {
  __shared__ uint64_t sm[kThreads / 64 + 1];
  const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanPer;
  uint64_t v[kScanPer], s = 0;
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    v[j] = base + j < n ? ld(base + j) : 0;
    s += v[j];
  }
  uint64_t total;
  uint64_t x = wg_excl_scan(s, sm, total) + tsum[blockIdx.x];
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    if (base + j < n) {
      out[base + j] = x;
      if (out2) out2[base + j] = x;
    }
    x += v[j];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = tsum[gridDim.x];
}

// The scan enqueued (n > 0); tsum_in and tsum are the caller's scratch.
template <class Load>
int scan(okv_ctx* ctx, DevBuf<uint64_t>& tsum_in, DevBuf<uint64_t>& tsum, Load ld, uint64_t n,
         uint64_t* out, uint64_t* out2) {
  const uint32_t ntiles = ceil_div(n, kScanTile);
  if (int rc = reserve(ctx, tsum, size_t(ntiles) + 1)) return rc;
  if (int rc = reserve(ctx, tsum_in, size_t(ntiles))) return rc;
  hipLaunchKernelGGL(okv_get_scan_sums_kernel<Load>, dim3(ntiles), dim3(kThreads), 0, ctx->stream,
                     ld, n, tsum_in.data());
  launch_scan_u64(ctx->stream, tsum_in.data(), ntiles, tsum.data(),
                  reinterpret_cast<unsigned long long*>(tsum.data() + ntiles));
  hipLaunchKernelGGL(okv_get_scan_write_kernel<Load>, dim3(ntiles), dim3(kThreads), 0, ctx->stream,
                     ld, n, tsum.data(), out, out2);
  OKV_HIP(hipGetLastError());
  return OKV_OK;
}

// ---- grouping: items into per-block lists, touched blocks into the work list.  tpos[i]
// is item i's block or kNone, gscan the scan of CntLoad over the nb blocks; a whole grid
// of kThreads-wide workgroups calls this. ------------------------------------------------
__device__ __forceinline__ void scatter_items(uint64_t n, uint64_t nb, const uint32_t* tpos,
                                              const uint64_t* gscan, uint32_t* cnt, uint32_t* list,
                                              uint32_t* work, uint64_t* blocks) {
  const uint64_t stride = uint64_t(gridDim.x) * kThreads;
  const uint64_t first = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  for (uint64_t i = first; i < n; i += stride) {
    const uint32_t t = tpos[i];
    if (t == kNone) continue;
    // (the count is taken down as the list fills: zero again for the next call)
    const uint32_t slot = uint32_t(gscan[t]) + atomicSub(&cnt[t], 1u) - 1u;
    list[slot] = uint32_t(i);
  }
  for (uint64_t t = first; t < nb; t += stride) {
    const uint64_t a = gscan[t], b = gscan[t + 1];
    if (uint32_t(a) != uint32_t(b)) work[uint32_t(a >> 32)] = uint32_t(t);
  }
  if (first == 0) *blocks = gscan[nb] >> 32;
}

// ---- search --------------------------------------------------------------------
template <uint32_t kCap>
struct __align__(16) SearchSmem {
  uint4 stage[(kCap + kStagePad) / 16];  // [16 B guard][block image][guard]
  uint16_t rec[kCap / 6 + 2];            // every record's position (< 64 KiB)
};

// One workgroup of kSearchThreads over the touched blocks w, w + gridDim.x, ...: the
// block staged into LDS by LDS DMA, ReadBlockWithStat's header walk by wave 0, then the
// block's items over the waves, lanes over the rows.  src says what a call's blocks and
// items are:
//   touched()                             blocks in the work list
//   block(w, seg, comp, d, k0, k1)        block w: its segment, descriptor and items
//                                         list[k0 .. k1); it passed go_read_status.
//                                         False: not a block of this search (a zstd
//                                         block: the inflate arms take it)
//   slot(w)                               block w's number among the call's blocks
//   item(j)                               list[j]
//   key(i, key, kl)                       item i's probe key
//   state, blk_status, val_off, val_len   per-item outputs
template <uint32_t kCap, class Src>
__device__ __forceinline__ void search_blocks(const Src& src_, SearchSmem<kCap>& sm, int32_t& s_st,
                                              uint32_t& s_rows) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t touched = src_.touched();
  for (uint32_t w = blockIdx.x; w < touched; w += gridDim.x) {
    const uint8_t* seg;
    int comp;
    Desc d;
    uint32_t k0, k1;
    // (the launch sized kCap for every block it takes)
    if (!src_.block(w, seg, comp, d, k0, k1) || d.block_size > kCap) continue;
    // the block passed go_read_status in the locate kernel: its BlockSize bytes are
    // in the segment.  Q7 (:331-333): the LZ4 flag decodes an empty buffer
    const uint32_t L = comp == OKV_COMP_LZ4 ? 0u : uint32_t(d.block_size);
    const Staged src{sm.stage, stage_block_wg<kSearchThreads>(sm.stage, seg, d.offset, L)};
    __syncthreads();
    if (tid < 64) {  // ReadBlockWithStat's record loop (:338-352) in full, by wave 0
      int32_t st = OKV_BLK_OK;
      uint64_t rows = 0, kb = 0, vb = 0, pend = 0;
      uint16_t* rec = sm.rec;
      walk_staged_to(src, L, d.original_size,
                     [rec](uint32_t row, uint32_t pos) { rec[row] = uint16_t(pos); }, lane, st,
                     rows, kb, vb, pend);
      if (lane == 0) {
        s_st = st;
        s_rows = uint32_t(rows);
      }
    }
    __syncthreads();
    const int32_t st = s_st;
    const uint32_t rows = s_rows;
    // the block's items over the waves; per item, lanes over the rows in block order
    for (uint32_t j = k0 + wave; j < k1; j += kSearchThreads / 64) {
      const uint32_t i = src_.item(j);
      if (st != OKV_BLK_OK) {  // a failed block fails its keys, wherever the bad record is
        if (lane == 0) {
          src_.state[i] = OKV_GET_BLOCK_ERROR;
          src_.blk_status[i] = st;
        }
        continue;
      }
      const uint8_t* key;
      uint32_t kl;
      src_.key(i, key, kl);
      uint32_t hit = kNone;
      for (uint32_t r0 = 0; r0 < rows; r0 += 64) {
        const uint32_t r = r0 + lane;
        const bool eq = r < rows && key_equal(src, sm.rec[r], kl, [key, kl](uint32_t b) {
                          return key_dword(key, kl, b);
                        });
        const uint64_t bm = __ballot(eq);
        if (bm) {  // the lowest matching row of the earliest round: the first in block order
          hit = r0 + uint32_t(__builtin_ctzll(bm));
          break;
        }
      }
      if (lane == 0 && hit != kNone) {
        const uint32_t pos = sm.rec[hit];
        uint32_t rkl, rvl;
        src.header(pos, rkl, rvl);
        src_.state[i] = OKV_GET_FOUND;
        src_.val_off[i] = d.offset + pos + 6 + rkl;
        src_.val_len[i] = rvl;
      }
    }
    __syncthreads();  // the stage and the positions are reused by the next block
  }
}

// ---- the inflate arms (OKV_F_GET_ZSTD) ----------------------------------------------
// The touched blocks of zstd segments: numbered and given room in one packed image
// (zplan_blocks), their CompressedSize bytes copied there (zpack_blocks), inflated by the
// zstd stage (zstd_stage: one call for the blocks of every segment), then searched from
// the stage's scratch: an inflated block of at most kStage bytes by search_blocks through
// ZSrc, a longer one from global memory (zglobal_blocks).
struct ZView {
  uint32_t on;               // the call has the flag and a zstd segment
  uint32_t* zidx;            // [blocks] a touched zstd block's number in the inflate batch
  unsigned long long* plan;  // [0] zstd blocks touched, [1] packed bytes, [2] blocks touched
  Desc* pdesc;               // [zstd blocks touched] into the packed image
  uint8_t* packed;
  const uint8_t* bytes;      // ZstdOut: the inflated blocks, their descriptors and statuses
  uint64_t n_bytes;
  const Desc* descs;
  const int32_t* status;
  uint32_t* rows;            // [n_bytes / 6 + 1] record positions of the global arm
  uint64_t* abs;             // [keys] a found value's offset in bytes (val_off: in its block)
};

// One lane per touched block.  A zstd block takes the next number and the next
// round16(CompressedSize) + 16 bytes of the packed image (so no offset is the image's
// end, which would read as io.EOF); its BlockSize there is CompressedSize: it covers the
// frames and nothing else.  The order is the atomics'; no result depends on it.
template <class Src>
__device__ __forceinline__ void zplan_blocks(const Src& s, const ZView& z) {
  const uint32_t touched = s.touched();
  const uint64_t first = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  for (uint64_t w = first; w < touched; w += uint64_t(gridDim.x) * kThreads) {
    const uint8_t* seg;
    int comp;
    Desc d;
    uint32_t k0, k1;
    if (s.block(uint32_t(w), seg, comp, d, k0, k1)) continue;
    const uint32_t zi = uint32_t(atomicAdd(&z.plan[0], 1ull));
    const uint64_t off = atomicAdd(&z.plan[1], (unsigned long long)(round16(d.compressed_size) + 16));
    z.zidx[s.slot(uint32_t(w))] = zi;
    z.pdesc[zi] = Desc{off, d.compressed_size, d.original_size, d.compressed_size};
  }
  if (first == 0) z.plan[2] = touched;
}

// One workgroup of kThreads per touched zstd block: its CompressedSize bytes (they are in
// the segment: locate_key checked BlockSize, and CompressedSize <= BlockSize) to its
// 16-byte-aligned place in the packed image, 16 bytes a lane.
template <class Src>
__device__ __forceinline__ void zpack_blocks(const Src& s, const ZView& z) {
  const uint32_t touched = s.touched();
  for (uint32_t w = blockIdx.x; w < touched; w += gridDim.x) {
    const uint8_t* seg;
    int comp;
    Desc d;
    uint32_t k0, k1;
    if (s.block(w, seg, comp, d, k0, k1)) continue;
    uint4* dst = reinterpret_cast<uint4*>(z.packed + z.pdesc[z.zidx[s.slot(w)]].offset);
    const uint64_t end = d.offset + d.compressed_size;
    for (uint64_t c = threadIdx.x; c < (d.compressed_size + 15) / 16; c += kThreads)
      dst[c] = window16(seg, end, int64_t(d.offset + 16 * c));
  }
}

// Work-list block w as the inflate arms see it: false when it is no zstd block, else its
// inflated image's descriptor (offset into z.bytes, BlockSize = the inflated length), the
// zstd stage's status and its items.
template <class Src>
__device__ __forceinline__ bool zblock(const Src& s, const ZView& z, uint32_t w, Desc& d,
                                       uint32_t& k0, uint32_t& k1, int32_t& st) {
  const uint8_t* seg;
  int comp;
  if (s.block(w, seg, comp, d, k0, k1)) return false;
  const uint32_t zi = z.zidx[s.slot(w)];
  d = z.descs[zi];
  st = z.status[zi];
  return true;
}

// search_blocks over the inflated blocks of at most kStage bytes: the stage's scratch is
// the segment, the inflated length the BlockSize (Go inflates every frame before its
// walk, so the walk's buffer is that length whatever OriginalSize says).  val_off comes
// out as an offset into z.bytes (zfix_value).
template <class Src>
struct ZSrc {
  const Src& s;
  const ZView& z;
  int32_t* state;
  int32_t* blk_status;
  uint64_t* val_off;
  uint32_t* val_len;
  __device__ __forceinline__ uint32_t touched() const { return s.touched(); }
  __device__ __forceinline__ bool block(uint32_t w, const uint8_t*& seg, int& comp, Desc& d,
                                        uint32_t& k0, uint32_t& k1) const {
    int32_t st;
    if (!zblock(s, z, w, d, k0, k1, st)) return false;
    seg = z.bytes, comp = OKV_COMP_NONE;
    return st == OKV_BLK_OK && d.block_size <= uint64_t(kStage);
  }
  __device__ __forceinline__ uint32_t item(uint32_t j) const { return s.item(j); }
  __device__ __forceinline__ void key(uint32_t i, const uint8_t*& key, uint32_t& kl) const {
    s.key(i, key, kl);
  }
};

struct GlobalBlock {  // walk_staged_to's byte source: a block in global memory
  const uint8_t* base;
  __device__ __forceinline__ void header(uint32_t pos, uint32_t& kl, uint32_t& vl) const {
    header_global(base, pos, kl, vl);
  }
};

// One workgroup of kSearchThreads per touched zstd block.  A block the decoder rejected
// fails its items (BLOCK_ERROR, the stage's status); one that inflated past
// OKV_GET_INFLATED_MAX sends them to FALLBACK; one of at most kStage bytes is the staged
// arm's.  Any other is searched here from global memory: wave 0 walks it (walk_staged_to
// over GlobalBlock) into the block's part of the row table -- rows + offset / 6: a block
// of L bytes has at most L / 6 records, and the blocks' regions are disjoint -- then the
// items go over the waves and the lanes over the rows, the first equal key in block order
// by ballot, as in search_blocks.
// walk_staged_to's u32 arithmetic holds unchanged for L <= OKV_GET_INFLATED_MAX = 2^24:
// pp <= L, and the record at pp passed its checks before the lanes spread, so
// kl <= 65535 and vl <= L and q = pp + lane * rl < 2^24 + 63 * (2^24 + 65541) < 2^31;
// every header is read at min(q, L) <= L, at most 12 bytes past the block (the stage's
// scratch has 64 bytes behind its last block).
template <class Src>
__device__ __forceinline__ void zglobal_blocks(const Src& s, const ZView& z, int32_t& s_st,
                                               uint32_t& s_rows) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t touched = s.touched();
  for (uint32_t w = blockIdx.x; w < touched; w += gridDim.x) {
    Desc d;
    uint32_t k0, k1;
    int32_t bst;
    if (!zblock(s, z, w, d, k0, k1, bst)) continue;
    if (bst != OKV_BLK_OK || d.block_size > uint64_t(OKV_GET_INFLATED_MAX)) {
      for (uint32_t j = k0 + tid; j < k1; j += kSearchThreads) {
        const uint32_t i = s.item(j);
        s.state[i] = bst != OKV_BLK_OK ? OKV_GET_BLOCK_ERROR : OKV_GET_FALLBACK;
        s.blk_status[i] = bst;
      }
      continue;
    }
    if (d.block_size <= uint64_t(kStage)) continue;
    const uint32_t L = uint32_t(d.block_size);
    const GlobalBlock g{z.bytes + d.offset};
    uint32_t* rec = z.rows + d.offset / 6;
    if (tid < 64) {  // ReadBlockWithStat's record loop (:338-352) in full, by wave 0
      int32_t st = OKV_BLK_OK;
      uint64_t rows = 0, kb = 0, vb = 0, pend = 0;
      walk_staged_to(g, L, d.original_size, RecSink{rec, L / 6}, lane, st, rows, kb, vb, pend);
      if (lane == 0) {
        s_st = st;
        s_rows = uint32_t(rows);
      }
    }
    __syncthreads();  // (the positions are global stores of this workgroup)
    const int32_t st = s_st;
    const uint32_t rows = s_rows;
    for (uint32_t j = k0 + wave; j < k1; j += kSearchThreads / 64) {
      const uint32_t i = s.item(j);
      if (st != OKV_BLK_OK) {
        if (lane == 0) {
          s.state[i] = OKV_GET_BLOCK_ERROR;
          s.blk_status[i] = st;
        }
        continue;
      }
      const uint8_t* key;
      uint32_t kl;
      s.key(i, key, kl);
      uint32_t hit = kNone;
      for (uint32_t r0 = 0; r0 < rows; r0 += 64) {
        const uint32_t r = r0 + lane;
        bool eq = false;
        if (r < rows) {  // bytes.Equal (:398) from global memory
          const uint32_t pos = rec[r];
          uint32_t rkl, rvl;
          g.header(pos, rkl, rvl);
          eq = rkl == kl;
          for (uint32_t b = 0; b < kl && eq; b += 4) {
            const uint32_t nb = min(4u, kl - b);
            const uint32_t m = nb == 4 ? ~0u : (1u << (8 * nb)) - 1u;
            eq = ((key_dword(g.base + pos + 6, kl, b) ^ key_dword(key, kl, b)) & m) == 0;
          }
        }
        const uint64_t bm = __ballot(eq);
        if (bm) {
          hit = r0 + uint32_t(__builtin_ctzll(bm));
          break;
        }
      }
      if (lane == 0 && hit != kNone) {
        const uint32_t pos = rec[hit];
        uint32_t rkl, rvl;
        g.header(pos, rkl, rvl);
        s.state[i] = OKV_GET_FOUND;
        s.val_off[i] = d.offset + pos + 6 + rkl;
        s.val_len[i] = rvl;
      }
    }
    __syncthreads();  // s_st and s_rows are reused by the next block
  }
}

// A found value of zstd block b (its number among the call's blocks): the searches left
// its offset in z.bytes in val_off[i]; that goes to abs[i] for the values kernel, and the
// caller gets the offset inside the inflated block.
__device__ __forceinline__ void zfix_value(const ZView& z, uint64_t i, uint32_t b,
                                           uint64_t* val_off) {
  const uint64_t a = val_off[i];
  z.abs[i] = a;
  val_off[i] = a - z.descs[z.zidx[b]].offset;
}

// ---- values ----------------------------------------------------------------------
// One wave: vl value bytes at seg + off into dst (16-byte aligned), 16 bytes a lane, the
// pad bytes of the last 16 zero.
__device__ __forceinline__ void copy_value(const uint8_t* seg, uint64_t seg_bytes, uint64_t off,
                                           uint32_t vl, uint4* dst, uint32_t lane) {
  for (uint32_t c = lane; c < (vl + 15) / 16; c += 64) {
    const uint4 v = window16(seg, seg_bytes, int64_t(off + 16ull * c));
    const int32_t nb = int32_t(min(16u, vl - 16 * c));
    dst[c] = merge_bytes(make_uint4(0, 0, 0, 0), v, 0, nb);
  }
}

// ---- host: what okv_get_rows and okv_snap_get_rows do alike.  S is the file's Scratch, P
// its Params, Out its okv_*_out; read is its read_totals (it synchronises). -----------
struct ZScratch {  // the inflate arms' part of a file's Scratch (its member z)
  DevBuf<uint32_t> zidx;
  DevBuf<unsigned long long> plan;
  PinBuf<unsigned long long> h_plan;
  DevBuf<Desc> pdesc;
  DevBuf<uint8_t> packed;
  DevBuf<uint32_t> rows;
  DevBuf<uint64_t> abs;
};
template <class P>
struct ZKernels {  // a file's kernels over zplan_blocks, zpack_blocks, ZSrc, zglobal_blocks
  void (*plan)(P);
  void (*pack)(P);
  void (*search_small)(P);
  void (*search_large)(P);
  void (*global)(P);
  uint64_t max_original;  // the largest OriginalSize of the call's indexes
  bool plain;             // the call may touch blocks that are not zstd
};

// The inflate arms behind the scatter (p.z.on): the plan, the one synchronisation that
// reads the touched counts, then the plain search for the other blocks, the pack, the zstd
// stage (it synchronises too) and the two searches of the inflated blocks.
template <class S, class P>
int inflate_and_search(okv_ctx* ctx, S* s, P& p, uint64_t most, uint64_t nb, uint32_t n_cu,
                       bool small, void (*search_small)(P), void (*search_large)(P),
                       const ZKernels<P>& zk) {
  ZScratch& z = s->z;
  if (int rc = reserve(ctx, z.zidx, size_t(nb))) return rc;
  if (int rc = reserve(ctx, z.plan, 3)) return rc;
  if (int rc = reserve(ctx, z.h_plan, 3)) return rc;
  if (int rc = reserve(ctx, z.pdesc, size_t(most))) return rc;
  p.z.zidx = z.zidx.data(), p.z.plan = z.plan.data(), p.z.pdesc = z.pdesc.data();
  OKV_HIP(hipMemsetAsync(p.z.plan, 0, 3 * sizeof(unsigned long long), ctx->stream));
  const uint32_t gp = std::max(1u, std::min(ceil_div(most, kThreads), n_cu * 8));
  hipLaunchKernelGGL(zk.plan, dim3(gp), dim3(kThreads), 0, ctx->stream, p);
  OKV_HIP(hipGetLastError());
  OKV_HIP(hipMemcpyAsync(z.h_plan.data(), p.z.plan, 3 * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, ctx->stream));
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  const uint64_t nz = z.h_plan.data()[0], zbytes = z.h_plan.data()[1];
  const uint64_t touched = z.h_plan.data()[2];
  if (zk.plain && touched > nz) {
    const uint32_t g = uint32_t(std::min<uint64_t>(touched, uint64_t(n_cu) * (small ? 8 : 2)));
    hipLaunchKernelGGL(small ? search_small : search_large, dim3(g), dim3(kSearchThreads), 0,
                       ctx->stream, p);
    OKV_HIP(hipGetLastError());
  }
  if (nz == 0) return OKV_OK;
  if (int rc = reserve(ctx, z.packed, size_t(zbytes) + 64)) return rc;
  p.z.packed = z.packed.data();
  const uint32_t gk = uint32_t(std::min<uint64_t>(touched, uint64_t(n_cu) * 8));
  hipLaunchKernelGGL(zk.pack, dim3(gk), dim3(kThreads), 0, ctx->stream, p);
  OKV_HIP(hipGetLastError());
  ZstdOut zo;
  if (int rc = zstd_stage(ctx, p.z.packed, zbytes, p.z.pdesc, uint32_t(nz), &zo)) return rc;
  ctx->last_path |= OKV_PATH_ZSTD | (zo.retried ? OKV_PATH_ZSTD_REGROW : 0u);
  // the row table from the stage's inflated total: rows <= L / 6 per block
  if (int rc = reserve(ctx, z.rows, size_t(zo.n_bytes / 6) + 2)) return rc;
  p.z.bytes = zo.bytes, p.z.n_bytes = zo.n_bytes, p.z.descs = zo.descs, p.z.status = zo.status;
  p.z.rows = z.rows.data();
  // the stage by the inflated sizes: without a regrow no block is longer than its first
  // region, round16(OriginalSize) at most
  const bool zsmall = !zo.retried && round16(zk.max_original) <= kSmallCap;
  const uint32_t g = uint32_t(std::min<uint64_t>(touched, uint64_t(n_cu) * (zsmall ? 8 : 2)));
  hipLaunchKernelGGL(zsmall ? zk.search_small : zk.search_large, dim3(g), dim3(kSearchThreads), 0,
                     ctx->stream, p);
  const uint32_t gg = uint32_t(std::min<uint64_t>(touched, uint64_t(n_cu) * 2));
  hipLaunchKernelGGL(zk.global, dim3(gg), dim3(kSearchThreads), 0, ctx->stream, p);
  OKV_HIP(hipGetLastError());
  return OKV_OK;
}

// The grouping and the search enqueued (nb > 0): cnt scanned over the nb blocks, the n
// items scattered into per-block lists, one workgroup per touched block with the stage
// max_block asks for.  zk (p.z.on): the inflate arms as well; the call then synchronises.
template <class S, class P>
int group_and_search(okv_ctx* ctx, S* s, P& p, uint64_t n, uint64_t nb, uint64_t max_block,
                     uint32_t n_cu, void (*scatter)(P), void (*search_small)(P),
                     void (*search_large)(P), const ZKernels<P>* zk = nullptr) {
  if (int rc = scan(ctx, s->tsum_in, s->tsum, CntLoad{p.cnt}, nb, p.gscan, nullptr)) return rc;
  const uint32_t gs = std::max(1u, std::min(ceil_div(std::max(n, nb), kThreads), n_cu * 8));
  hipLaunchKernelGGL(scatter, dim3(gs), dim3(kThreads), 0, ctx->stream, p);
  const bool small = max_block <= kSmallCap;
  const uint64_t most = std::min(n, nb);  // touched blocks at most
  if (zk)
    return inflate_and_search(ctx, s, p, most, nb, n_cu, small, search_small, search_large, *zk);
  const uint32_t g = uint32_t(std::min<uint64_t>(most, uint64_t(n_cu) * (small ? 8 : 2)));
  hipLaunchKernelGGL(small ? search_small : search_large, dim3(g), dim3(kSearchThreads), 0,
                     ctx->stream, p);
  OKV_HIP(hipGetLastError());
  return OKV_OK;
}

// What a call does first: the arena and capacity okv_*_totals judges by and, for an
// empty call (n == 0: nothing is launched), this call's totals: none.
template <class S, class Out>
int open_call(okv_ctx* ctx, S* s, const Out* out, uint64_t n) {
  s->last_arena = out->val_arena != nullptr;
  s->last_cap = out->val_cap;
  if (n || !s->d_tot.data()) return OKV_OK;
  OKV_HIP(hipSetDevice(ctx->device));
  OKV_HIP(hipMemsetAsync(s->d_tot.data(), 0, sizeof(*s->d_tot.data()), ctx->stream));
  return OKV_OK;
}

// okv_*_totals after the caller zeroed *out: the last call's totals and its capacity error.
template <class S, class Out, class Read>
int last_totals(okv_ctx* ctx, S* s, Out* out, const char* cap_msg, Read read) {
  if (!s || !s->d_tot.data()) return OKV_OK;  // no call has launched anything
  OKV_HIP(hipSetDevice(ctx->device));
  if (int rc = reserve(ctx, s->h_tot, 1)) return rc;
  if (int rc = read(ctx, s, out)) return rc;
  if (s->last_arena && out->val_bytes > s->last_cap) return set_err(ctx, OKV_E_CAPACITY, cap_msg);
  return OKV_OK;
}

// After run(): the values and the totals.  Device mode: the values kernel behind run()
// (it writes nothing when they do not fit), then, unless OKV_F_ASYNC, the totals.  Host
// mode: the columns back, the totals, and when the values fit a device arena of exactly
// val_bytes, the values kernel and the copy out.  values(p) launches the values kernel.
template <class S, class P, class Out, class Read, class Values>
int finish_values(okv_ctx* ctx, S* s, P& p, Out* out, uint32_t flags, const stage::Col* cols,
                  size_t ncols, const char* cap_msg, Read read, Values values) {
  const bool dev = flags & OKV_F_DEVICE_PTRS;
  if (dev) {
    if (out->val_arena)
      if (int rc = values(p)) return rc;
    if (flags & OKV_F_ASYNC) return OKV_OK;
  } else if (int rc = stage_out(ctx, cols, ncols, p.n)) {
    return rc;
  }
  if (int rc = read(ctx, s, out)) return rc;
  if (!out->val_arena) return OKV_OK;
  if (out->val_bytes > out->val_cap) return set_err(ctx, OKV_E_CAPACITY, cap_msg);
  if (dev || out->val_bytes == 0) return OKV_OK;
  if (int rc = reserve(ctx, s->d_val, size_t(out->val_bytes))) return rc;
  p.val_arena = s->d_val.data();
  p.val_cap = out->val_bytes;
  if (int rc = values(p)) return rc;
  OKV_HIP(hipMemcpyAsync(out->val_arena, p.val_arena, out->val_bytes, hipMemcpyDeviceToHost,
                         ctx->stream));
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  return OKV_OK;
}

}  // namespace
}  // namespace get
}  // namespace okv
