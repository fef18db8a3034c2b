// okv_decode.hip -- MI355X (gfx950) batched SST data-block decode.
//
// Replaces the record loop of sst.SegmentReader.ReadBlockWithStat
// (/root/reference/sst/segment_reader.go:295-355) for many blocks at once.
// Launches per call:
//   1. okv_count_kernel  -- one lane per block walks the record headers in
//      HBM, validating exactly what the Go loop validates; per block it emits
//      (status, rows, key bytes, value bytes, end position), the positions and
//      key lengths of its first kRCap records (block-major table, written
//      through LDS in whole 16-byte pieces) and a 256-block exclusive scan.
//      Blocks with more rows go on the "big block" list.  Pass 2 runs in the
//      same launch: the workgroup that arrives last scans the tile totals
//      (sc1 hand-off), so a decode needs no memset and no scan launch.
//   2. pass 3, by the call's average block span:
//      okv_tile_kernel (> 16 KiB, the C3/C5 kernel) -- one workgroup per
//        16 KiB source tile of a block: the tile's bytes are DMA'd into LDS
//        while wave 0 rebuilds the row table from pass 1's record table; whole
//        value chunks go out as wave-uniform runs, keys and the chunks that
//        mix rows by a per-lane lookup; tile 0 writes the SoA row index.
//      okv_gather_small_kernel (<= 16 KiB blocks) -- one wave per block, the
//        whole block staged in LDS.
//      okv_decode_fused_kernel (<= 512 small blocks) -- passes 1-3 in one
//        launch (replaces 1 and 2 as well).
//   3. okv_copy_kernel   -- persistent, over the big-block list only: stages
//      the block in LDS and chases its headers there (rare: > kRCap rows).
// OKV_F_INDEX_ONLY writes spans into seg instead of arenas (+ okv_index_kernel).
// Measured alternatives to pass 3 are in DESIGN.md §4 and the ablation build
// (-DOKV_ABLATE).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "okv_ctx.hpp"
#include "okv_kernels.hpp"
#include "okv_sst.h"

namespace okv {

// Record table from pass 1, block-major: record r < kRCap of block b at
// rt_pos[b * kRCap + r] (u32 position in the block) and rt_kl[b * kRCap + r]
// (u16 key length).  A consumer wave reads a block's table with one
// coalesced 256-B (128-B) load.  Pass 1 buffers kRecChunk records per lane
// in LDS and writes them out as whole 16-byte pieces (see okv_count_kernel).
__device__ __forceinline__ uint64_t rec_index(uint32_t /*nblk*/, uint32_t b, uint32_t r) {
  return uint64_t(b) * kRCap + r;
}
constexpr uint32_t kRecChunk = 16;  // records per lane between two LDS flushes

// ---------------------------------------------------------------------------
// Pass 1: header walk in HBM, one lane per block.
// ---------------------------------------------------------------------------
// Small segments (prefetch = 1): each lane first touches one dword per 128-B
// line of its block's record bytes -- independent loads, all in flight at
// once -- so the dependent header chase then hits the caches instead of HBM.
// A single-tile launch (one workgroup) also zeroes the big-block counter and
// writes the totals itself (no memset, no scan launch): single_* non-null.
//
// Record table: every kRecChunk steps of the walk the workgroup stops at a
// barrier and writes the slots its lanes recorded since the last stop, as
// whole 16-byte pieces of the block-major table (4 consecutive lanes write
// one block's 64 bytes of positions).  Lockstep per-lane stores into a
// strided table (round 2: [r/16][block][r%16], u32 positions + u64 headers)
// left partial lines that the walk's own reads evicted between steps: 136 MB
// written per C3 launch for 50 MB of slots.
//
// Big blocks (okv_copy_kernel): more than kRCap rows, a walk ending at or past
// 4 GiB, or past span_cap (the tile pass's span: okv_tile_kernel).
__global__ __launch_bounds__(kThreads) void okv_count_kernel(
    const uint8_t* __restrict__ seg, uint64_t seg_bytes, const Desc* __restrict__ descs,
    uint32_t nblk, int comp, BlockCount* __restrict__ cnt, Prefix* __restrict__ lp,
    Prefix* __restrict__ tile_tot, uint32_t* __restrict__ rt_pos, uint16_t* __restrict__ rt_kl,
    uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count,
    const int32_t* __restrict__ pre_status, int prefetch, uint64_t span_cap,
    Prefix* __restrict__ tile_pre, Totals* __restrict__ tot, uint64_t* __restrict__ row_start,
    uint32_t* __restrict__ arrive, uint32_t* __restrict__ big_zero,
    const Totals* __restrict__ base, uint32_t bidx0, unsigned long long* __restrict__ span_max) {
  // slots of the current chunk: positions [lane][kRecChunk + 1] (odd stride:
  // the walking lanes' stores hit distinct banks), key lengths [lane][kRecChunk]
  __shared__ uint32_t s_pos[kThreads * (kRecChunk + 1)];
  __shared__ __align__(16) uint16_t s_kl[kThreads * kRecChunk];
  __shared__ uint32_t s_rows[kThreads];
  const uint32_t tid = threadIdx.x;
  const uint32_t b = blockIdx.x * kTile + tid;
  uint64_t rows = 0, kb = 0, vb = 0, p = 0;
  int32_t st = OKV_BLK_OK;
  // the other big-block counter slot, for the next launch (its readers, the
  // previous decode's kernels, have completed: stream order)
  if (blockIdx.x == 0 && tid == 0 && big_zero) *big_zero = 0;
  uint64_t len = 0, orig = 0, off = 0;
  bool walking = false;
  if (b < nblk) {
    const Desc d = descs[b];
    const int32_t pre = pre_status ? pre_status[b] : int32_t(OKV_BLK_OK);
    if (pre != OKV_BLK_OK) {
      st = pre;  // outcome of the zstd stage (raw-block bounds, decoder error)
    } else if ((st = go_read_status(d, seg_bytes)) != OKV_BLK_OK) {
      // Seek error / makeslice panic / io.EOF / ErrUnexpectedBytesRead (:303-316)
    } else if (comp == OKV_COMP_ZSTD) {
      st = OKV_BLK_UNSUPPORTED;  // index-only spans cannot point into decompressed bytes
    } else {
      len = (comp == OKV_COMP_LZ4) ? 0 : d.block_size;  // Q7 (:331-333)
      orig = go_walk_bound(d.original_size);  // int(OriginalSize) < 0: no iteration (:340)
      off = d.offset;
      walking = true;
      if (prefetch && orig && len) {
        // up to 32 lines (4 KiB), all issued before any is waited on;
        // addresses clamped into [offset, offset + min(orig, len))
        const uint64_t first = off & ~uint64_t(3);
        const uint64_t last = (off + (orig < len ? orig : len) - 1) & ~uint64_t(3);
        uint32_t v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
          uint64_t a = (off & ~uint64_t(127)) + 128ull * u;
          a = a < first ? first : (a > last ? last : a);
          v[u] = *reinterpret_cast<const uint32_t*>(seg + a);
        }
        uint32_t acc = 0;
#pragma unroll
        for (int u = 0; u < 32; ++u) acc ^= v[u];
        asm volatile("" ::"v"(acc));  // keep the loads; their values are unused
      }
    }
  }
  // The walk is a dependent chain (record i+1 starts where i ends), so this
  // kernel is bound by HBM latency x the longest block's row count.
  const uint32_t b0 = blockIdx.x * kTile;
  for (uint32_t c = 0; c < uint32_t(kRCap) / kRecChunk; ++c) {
    const uint64_t cap = uint64_t(c + 1) * kRecChunk;
    if (walking) {
      while (p < orig && rows < cap) {  // :340
        if (len - p < 6) { st = OKV_BLK_PANIC; break; }  // u16/u32 reads (:342-345)
        uint32_t kl, vl;
        header_global(seg, off + p, kl, vl);
        const uint64_t room = len - p - 6;
        if (kl > room || vl > room - kl) {  // zero-length reads always succeed (:490-493)
          st = OKV_BLK_PANIC;                // key/value reads (:346-349)
          break;
        }
        const uint32_t slot = uint32_t(rows) & (kRecChunk - 1);
        s_pos[tid * (kRecChunk + 1) + slot] = uint32_t(p);
        s_kl[tid * kRecChunk + slot] = uint16_t(kl);
        rows++;
        kb += kl;
        vb += vl;
        p += 6 + uint64_t(kl) + uint64_t(vl);
      }
      if (st != OKV_BLK_OK) walking = false;
    }
    s_rows[tid] = st == OKV_BLK_OK ? uint32_t(rows) : 0u;
    __syncthreads();
    // slots [c * 16, c * 16 + 16) of the workgroup's blocks, live ones only
    for (uint32_t q = tid; q < uint32_t(kTile) * 4; q += kThreads) {
      const uint32_t lb = q >> 2, sub = q & 3, slot = c * kRecChunk + sub * 4;
      if (b0 + lb < nblk && slot < s_rows[lb]) {
        const uint32_t* s = &s_pos[lb * (kRecChunk + 1) + sub * 4];
        *reinterpret_cast<uint4*>(rt_pos + rec_index(nblk, b0 + lb, slot)) =
            make_uint4(s[0], s[1], s[2], s[3]);
      }
    }
    if (rt_kl) {
      for (uint32_t q = tid; q < uint32_t(kTile) * 2; q += kThreads) {
        const uint32_t lb = q >> 1, sub = q & 1, slot = c * kRecChunk + sub * 8;
        if (b0 + lb < nblk && slot < s_rows[lb])
          *reinterpret_cast<uint4*>(rt_kl + rec_index(nblk, b0 + lb, slot)) =
              *reinterpret_cast<const uint4*>(&s_kl[lb * kRecChunk + sub * 8]);
      }
    }
    walking = walking && p < orig;  // (then rows == cap)
    if (!__syncthreads_or(walking)) break;  // also the barrier before the slots are reused
  }
  // blocks with more than kRCap rows: finish the walk without recording
  if (walking) {
    while (p < orig) {
      if (len - p < 6) { st = OKV_BLK_PANIC; break; }
      uint32_t kl, vl;
      header_global(seg, off + p, kl, vl);
      const uint64_t room = len - p - 6;
      if (kl > room || vl > room - kl) { st = OKV_BLK_PANIC; break; }
      rows++;
      kb += kl;
      vb += vl;
      p += 6 + uint64_t(kl) + uint64_t(vl);
    }
  }
  if (b < nblk) {
    if (st != OKV_BLK_OK) rows = kb = vb = 0;
    if (st == OKV_BLK_OK && (rows > kRCap || p >= (uint64_t(1) << 32) || p > span_cap))
      big_list[atomicAdd(big_count, 1u)] = bidx0 + b;  // staged path (okv_copy_kernel)
    BlockCount c;
    c.rows = rows;
    c.kbytes = kb;
    c.vbytes = vb;
    c.pend = p;
    c.status = st;
    c.pad = 0;
    cnt[b] = c;
  }
  if (span_max) {  // the longest walk (okv_decode_plan: the tile pass's span hint)
    unsigned long long m = b < nblk && st == OKV_BLK_OK ? p : 0ull;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(m, d, 64);
      m = o > m ? o : m;
    }
    if ((tid & 63) == 0 && m) atomicMax(span_max, m);
  }
  // workgroup exclusive scan of (rows, padded kb, padded vb, bad)
  __shared__ uint64_t s_w[4][kThreads / 64];
  const int lane = tid & 63, wave = tid >> 6;
  uint64_t v[4] = {rows, round16(kb), round16(vb), uint64_t(b < nblk && st != OKV_BLK_OK)};
  uint64_t inc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    inc[k] = wave_incl_scan(v[k], lane);
    if (lane == 63) s_w[k][wave] = inc[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint64_t off2 = 0;
    for (int w = 0; w < wave; ++w) off2 += s_w[k][w];
    inc[k] += off2 - v[k];  // exclusive
  }
  if (b < nblk) {
    Prefix e;
    e.rows = inc[0];
    e.kb = inc[1];
    e.vb = inc[2];
    e.bad = inc[3];
    lp[b] = e;
  }
  // Pass 2 in the same launch: the workgroup whose arrival is counted last
  // scans the tile totals.  Hand-off (MI355X_MICROARCH.md, inter-workgroup
  // hand-off table, row 1): one lane per workgroup stores its totals with sc1
  // stores, drains them (vmcnt(0)), then adds to one unsharded agent-scope
  // counter; the workgroup whose add came last (told by the value it returns)
  // reads every total with sc1 loads.  Round 4 made the add a release and
  // the last adder acquire: an L2 write-back per workgroup of the ~66 KB of
  // record table each has just written -- 6.5 us more per C3 count (A/B,
  // profiles/r5/session/ab_count_arrival.log).  The totals travel write-
  // through (sc1 stores, drained before the add), so no producer needs a
  // release; the last adder still takes an agent-scope acquire before its
  // loads (one L1 invalidate, in one workgroup), so the loads are ordered
  // after the add by the memory model, not only by the sc1 load path.
  __shared__ uint32_t s_last;
  if (tid == kThreads - 1) {
    const Prefix t{inc[0] + v[0], inc[1] + v[1], inc[2] + v[2], inc[3] + v[3]};
    if (gridDim.x == 1) {
      const Totals b0 = base ? *base : Totals{0, 0, 0, 0};
      *tile_pre = Prefix{b0.rows, b0.kb, b0.vb, b0.bad};
      *tot = Totals{b0.rows + t.rows, b0.kb + t.kb, b0.vb + t.vb, b0.bad + t.bad};
      if (row_start) row_start[nblk] = b0.rows + t.rows;
      s_last = 0;
    } else {
      Prefix* q = tile_tot + blockIdx.x;
      __hip_atomic_store(&q->rows, t.rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&q->kb, t.kb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&q->vb, t.vb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&q->bad, t.bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const uint32_t a =
          __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = a == gridDim.x - 1;
    }
  }
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  // the last workgroup: exclusive scan of gridDim.x tile totals, 256 at a time
  // (from the totals of the blocks before this launch's, for a decode in pieces)
  uint64_t carry[4] = {0, 0, 0, 0};
  if (base) {
    carry[0] = base->rows;
    carry[1] = base->kb;
    carry[2] = base->vb;
    carry[3] = base->bad;
  }
  for (uint32_t base = 0; base < gridDim.x; base += kThreads) {
    const uint32_t i = base + tid;
    uint64_t x[4] = {0, 0, 0, 0};
    if (i < gridDim.x) {
      const Prefix* q = tile_tot + i;
      x[0] = __hip_atomic_load(&q->rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      x[1] = __hip_atomic_load(&q->kb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      x[2] = __hip_atomic_load(&q->vb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      x[3] = __hip_atomic_load(&q->bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    uint64_t in[4];
    __syncthreads();  // s_w reuse
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      in[k] = wave_incl_scan(x[k], lane);
      if (lane == 63) s_w[k][wave] = in[k];
    }
    __syncthreads();
    uint64_t sum[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint64_t o = carry[k];
      for (int w = 0; w < wave; ++w) o += s_w[k][w];
      in[k] += o - x[k];  // exclusive
      sum[k] = s_w[k][0] + s_w[k][1] + s_w[k][2] + s_w[k][3];
    }
    if (i < gridDim.x) tile_pre[i] = Prefix{in[0], in[1], in[2], in[3]};
#pragma unroll
    for (int k = 0; k < 4; ++k) carry[k] += sum[k];
  }
  if (tid == 0) {
    *tot = Totals{carry[0], carry[1], carry[2], carry[3]};
    if (row_start) row_start[nblk] = carry[0];
    // every workgroup has added: reset the counter for the next launch
    __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------
// Pass 3: per-block materialisation.
// ---------------------------------------------------------------------------
struct CopyParams {
  const uint8_t* seg;
  uint64_t seg_bytes;
  const Desc* descs;
  uint32_t nblk;
  int comp;
  int index_only;
  const BlockCount* cnt;
  const Prefix* lp;
  const Prefix* tile_pre;
  const uint32_t* rt_pos;     // pass-1 record table: positions (block-major, rec_index)
  const uint16_t* rt_kl;      // ... and key lengths (null unless the pass needs them)
  uint32_t* big_list;         // blocks with > kRCap rows (or >= 4 GiB walks)
  uint32_t* big_count;
  uint64_t* row_start;
  uint64_t* key_base;
  uint64_t* val_base;
  int32_t* blk_status;
  uint64_t* key_off;
  uint16_t* key_len;
  uint64_t* val_off;
  uint32_t* val_len;
  uint8_t* key_arena;
  uint8_t* val_arena;
  uint64_t row_cap, key_cap, val_cap;
  // value sweep hand-off (okv_value_sweep_kernel; null: pass 3 gathers values itself)
  uint64_t* vsrc;             // [row] segment position of the row's value
  uint32_t* vtile;            // [value-arena tile] row owning the tile's first byte
  uint4* bchunk;              // [row] the chunk holding the end of the row's value
  const Totals* tot;          // call totals (pass 1 / pass 2)
  uint64_t span_cap;          // okv_tile_kernel: blocks whose walk ends past it are big
};

// Global row / arena bases of block b and its final status (capacity check).
struct BlockBase {
  uint64_t row0, kb0, vb0;
  int32_t st;
};
__device__ __forceinline__ BlockBase block_base_of(const CopyParams& P, const BlockCount& c,
                                                   const Prefix& l, const Prefix& t) {
  BlockBase r;
  r.row0 = t.rows + l.rows;
  r.kb0 = t.kb + l.kb;
  r.vb0 = t.vb + l.vb;
  r.st = c.status;
  if (r.st == OKV_BLK_OK &&
      (r.row0 + c.rows > P.row_cap ||
       (!P.index_only && (r.kb0 + round16(c.kbytes) > P.key_cap ||
                          r.vb0 + round16(c.vbytes) > P.val_cap))))
    r.st = OKV_BLK_CAPACITY;
  return r;
}
__device__ __forceinline__ BlockBase block_base(const CopyParams& P, uint32_t b,
                                                const BlockCount& c) {
  return block_base_of(P, c, P.lp[b], P.tile_pre[b / kTile]);
}

// Lanes per row for a region whose rows average `avg` bytes.
__device__ __forceinline__ uint32_t group_size(uint64_t avg) {
  const uint64_t chunks = avg / 16 + 2;
  uint32_t g = 1;
  while (g < 64 && g < chunks) g <<= 1;
  return g;
}

struct GatherSmem {
  uint32_t rec[kRCap + 1];   // record position within the block
  uint32_t kpre[kRCap + 1];  // exclusive prefix of key lengths (kpre[rows] = total)
  uint32_t vpre[kRCap + 1];  // exclusive prefix of value lengths
  uint32_t ksb[kRCap];       // source of key-region byte x of row r = off + ksb[r] + x
  uint32_t vsb[kRCap];       // likewise for values
};

// Byte source for the gather: the segment in HBM (two aligned 16-byte loads +
// funnel).  rel = position relative to the block start (may be a few bytes
// negative for windows that begin before a row: those bytes are masked off).
struct GlobalWin {
  const uint8_t* seg;
  uint64_t seg_bytes;
  uint64_t off;
  __device__ __forceinline__ uint4 at(int64_t rel) const {
    return window16(seg, seg_bytes, int64_t(off) + rel);
  }
  __device__ __forceinline__ void header(uint32_t pos, uint32_t& kl, uint32_t& vl) const {
    header_global(seg, off + pos, kl, vl);
  }
};
// Gather one arena region (keys or values) of a block.  Each wave streams
// contiguous 1 KiB destination tiles: lane l of tile t writes chunk 64t + l
// (16 bytes, dwordx4).  The row holding the chunk's first byte is found by
// binary search on the lane's first chunk and by linear advance after
// (chunks only move forward).  A chunk that spills past its row is completed
// in registers from the following rows; past the region end it is zero (the
// 16-byte padding).  kU tiles per iteration keep kU windows in flight per lane.
// Tiles t0, t0 + ts, ... (< t1) of a region.
template <bool kVal, class Src, uint32_t kU = 4>
__device__ __forceinline__ void gather_tiles(const Src& src, const GatherSmem& sm, int rows,
                                             uint8_t* __restrict__ arena, uint64_t dbase,
                                             uint32_t t0, uint32_t t1, uint32_t ts) {
  const uint32_t* pre = kVal ? sm.vpre : sm.kpre;
  const uint32_t* sb = kVal ? sm.vsb : sm.ksb;
  const uint32_t total = pre[rows];
  const uint32_t N = (total + 15) >> 4;  // chunks, including the padded tail
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t last = uint32_t(rows) - 1;
  const uint32_t cmax = (N < t1 * 64 ? N : t1 * 64) - 1;  // last chunk of the range (ts == 1)
  for (uint32_t t = t0; t < t1; t += kU * ts) {
    uint4 v[kU];
    uint32_t rr[kU];
    // phase 1: rows and addresses; issue every load before any data is used
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint32_t c = (t + u * ts) * 64 + lane;
      const bool ok = (t + u * ts) < t1 && c < N;
      // lanes past the range reload the range's last chunk (an address a
      // valid lane loads in this iteration).  Pointing them at the range's
      // first tile with the current row's bias re-fetched ~40 evicted lines
      // per block (0.32 GB at C3).
      const uint32_t x = (ok ? c : cmax) << 4;
      // the row holding byte x: r = #{k in [1, rows) : pre[k] <= x}, a binary
      // search per chunk (pre[rows] = total > x ends every probe past the
      // last row).  The kU searches are independent, so their LDS reads
      // overlap; advancing linearly from the previous chunk's row cost one
      // dependent read per row passed (16 per tile for 64-byte rows).
      uint32_t r = 0;
#pragma unroll
      for (uint32_t st = 64; st; st >>= 1) {
        const uint32_t j = r + st;
        r = pre[min(j, last + 1)] <= x ? j : r;
      }
      rr[u] = r;
      v[u] = src.at(int64_t(sb[r]) + int64_t(x));
    }
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint32_t c = (t + u * ts) * 64 + lane;
      if ((t + u * ts) < t1 && c < N) {
        const uint32_t x = c << 4, xe = x + 16;
        uint4 out = v[u];
        const uint32_t ri = rr[u];
        if (xe > pre[ri + 1]) {  // spills past row ri (or past the region end)
          out = merge_bytes(make_uint4(0, 0, 0, 0), out, 0, int32_t(pre[ri + 1] - x));
          for (uint32_t j = ri + 1; j <= last && pre[j] < xe; ++j) {
            const uint32_t q0 = pre[j], q1 = pre[j + 1];
            if (q1 == q0) continue;
            const uint4 w = src.at(int64_t(sb[j]) + int64_t(x));
            out = merge_bytes(out, w, int32_t(q0 - x), int32_t((q1 < xe ? q1 : xe) - x));
          }
        }
        *reinterpret_cast<uint4*>(arena + dbase + uint64_t(x)) = out;
      }
    }
  }
}

// Tiles of a region split over nw waves in contiguous ranges.  Measured (C3,
// DESIGN.md §4): interleaving the tiles over the waves, 2 or 8 tiles per
// iteration, prefetching a spilling chunk's next-row window with the first
// (+11 VGPRs: 4 waves/SIMD instead of 5) and forcing 6-8 waves/SIMD (spills)
// are all slower.
template <bool kVal, class Src>
__device__ __forceinline__ void gather_region(const Src& src, const GatherSmem& sm, int rows,
                                              uint8_t* __restrict__ arena, uint64_t dbase,
                                              uint32_t wave, uint32_t nw) {
  const uint32_t T = ((kVal ? sm.vpre : sm.kpre)[rows] + 1023) >> 10;  // 1 KiB tiles
  gather_tiles<kVal, Src>(src, sm, rows, arena, dbase, uint32_t(uint64_t(T) * wave / nw),
                          uint32_t(uint64_t(T) * (wave + 1) / nw), 1);
}

// Per-block metadata every gather kernel starts from.
struct BlockMeta {
  BlockCount c;
  BlockBase B;
  uint64_t off;
};
__device__ __forceinline__ BlockMeta block_meta(const CopyParams& P, uint32_t b) {
  BlockMeta m;
  m.c = P.cnt[b];
  m.B = block_base(P, b, m.c);
  m.off = P.descs[b].offset;
  return m;
}
// Block outcome (tid 0) and whether the gather kernels handle its rows
// (else: nothing to do, or a big block for okv_copy_kernel / okv_index_kernel).
__device__ __forceinline__ bool block_head(const CopyParams& P, uint32_t b, const BlockMeta& m) {
  if (threadIdx.x == 0) {
    P.row_start[b] = m.B.row0;
    if (P.key_base) P.key_base[b] = m.B.kb0;
    if (P.val_base) P.val_base[b] = m.B.vb0;
    P.blk_status[b] = m.B.st;
  }
  return m.B.st == OKV_BLK_OK && m.c.rows != 0 && m.c.rows <= uint64_t(kRCap) &&
         m.c.pend < (uint64_t(1) << 32);
}

// Row table (wave 0, lane r = row r): wave scans give each row's key/value
// prefix and its source bias.
__device__ __forceinline__ void fill_row_table(GatherSmem& sm, int rows, uint32_t rec,
                                               uint32_t kl, uint32_t vl) {
  const uint32_t tid = threadIdx.x & 63;
  const uint32_t ki = wave_incl_scan32(kl, tid), vi = wave_incl_scan32(vl, tid);
  if (int(tid) < rows) {
    sm.rec[tid] = rec;
    sm.kpre[tid] = ki - kl;
    sm.vpre[tid] = vi - vl;
    sm.ksb[tid] = rec + 6 - (ki - kl);       // >= 0: earlier keys precede rec
    sm.vsb[tid] = rec + 6 + kl - (vi - vl);  // >= 0: earlier values precede rec
    if (int(tid) == rows - 1) {
      sm.rec[rows] = rec + 6 + kl + vl;
      sm.kpre[rows] = ki;
      sm.vpre[rows] = vi;
    }
  }
}
// ... from headers read at the pass-1 positions
template <class Src>
__device__ __forceinline__ void build_row_table(const Src& src, GatherSmem& sm, int rows,
                                                uint32_t rec) {
  uint32_t kl = 0, vl = 0;
  if (int(threadIdx.x & 63) < rows) src.header(rec, kl, vl);
  fill_row_table(sm, rows, rec, kl, vl);
}
// SoA row index of a block (lane r = row r).
__device__ __forceinline__ void write_row_index(const CopyParams& P, const GatherSmem& sm,
                                                const BlockMeta& m, int rows) {
  const uint32_t tid = threadIdx.x;
  if (int(tid) >= rows) return;
  const uint64_t g = m.B.row0 + tid;
  const uint32_t kl = sm.kpre[tid + 1] - sm.kpre[tid], vl = sm.vpre[tid + 1] - sm.vpre[tid];
  P.key_len[g] = uint16_t(kl);
  P.val_len[g] = vl;
  if (P.index_only) {
    P.key_off[g] = m.off + sm.rec[tid] + 6;
    P.val_off[g] = m.off + sm.rec[tid] + 6 + kl;
  } else {
    P.key_off[g] = m.B.kb0 + sm.kpre[tid];
    P.val_off[g] = m.B.vb0 + sm.vpre[tid];
  }
}

// ---------------------------------------------------------------------------
// Pass 3, source tiles (large blocks).  Block b is cut into
// tiles of kT source bytes, tile t = block bytes [t kT, (t + 1) kT), one
// short-lived 256-thread workgroup each, dispatched in address order: the
// whole chip's loads and stores stay in one compact window of the segment
// and the arenas (the one-shot copy shape).  A workgroup
//   1. loads the block's metadata and its pass-1 record table (one trip),
//   2. DMAs its tile (plus a 16-byte lead-in and a guard line) into LDS with
//      global_load_lds_dwordx4 -- the only read of the record bytes,
//   3. writes every key and value byte whose SOURCE lies in its tile: the
//      destination ranges are contiguous (rows are packed in record order),
//      each 16-byte destination chunk is assembled from the stage (one LDS
//      window per row piece) and stored whole; the two chunks at a range's
//      ends that the neighbouring tile shares are stored byte-exactly
//      (store_partial: disjoint bytes, no read-modify-write).
// The value-range cut between two tiles of a block moves up to the next
// 128-byte line of the arena when the bytes it adds lie in the tile's staged
// extension (kLineExt source bytes past its end): stores from two workgroups
// never share that line.  (Every store instruction that covers part of a
// 64-byte sector costs the HBM a whole 64-byte write request -- the L2 does
// not merge separate stores into one; PMC by output class)
// Tile 0 also writes the block's row index (SoA) and its block outputs.  The
// last tile writes the zero padding of the block's arena regions.  Each
// source byte is read once and each arena byte written once, so the pass
// moves its algorithmic bytes: the round-2 row pass + value sweep read the
// lines values share with headers and keys twice (1.11x).
// kXcd: consecutive tiles run on one XCD (hardware deals workgroups to the 8
// XCDs round-robin), so a block's metadata and the chunks two tiles share
// meet in one L2.
// ---------------------------------------------------------------------------
template <uint32_t kUnits>
struct TileRowsT {
  uint32_t pre[2][kRCap + 1];  // [key, value] exclusive prefix of lengths (pre[rows] = total)
  uint32_t sb[2][kRCap];       // block position of region byte x of row r = sb[r] + x
  uint32_t x[4];               // owned key range [x0, x1), value range [x2, x3)
  // value runs (kRuns): whole value chunks in units of <= 64 inside one
  // row piece {dest chunk, stage byte of its first chunk, count}, and the
  // value chunks that mix rows, padding or a neighbouring tile's bytes
  uint32_t unit[3][kUnits];
  uint32_t bnd[2 * kRCap + 4];  // (sector form: up to two mixed sectors per row)
  uint32_t nunit, nbnd;
};
// value runs of a kT-byte tile: at most one partial run per row plus kT / 1 KiB
// whole ones (16 KiB tiles: 96 entries, as before)
template <uint32_t kT>
using TileRows = TileRowsT<(kT / 1024 + kRCap + 16 + 15) & ~15u>;

// 16 bytes at byte s (0..15, wave-uniform) of the 32-byte window (x, y): a
// scalar branch picks the dwords, then 4 v_alignbyte.
__device__ __forceinline__ uint4 funnel_u(const uint4& x, const uint4& y, uint32_t s) {
  const uint32_t r = s & 3;
  switch (s >> 2) {
    case 0:
      return make_uint4(funnel(x.y, x.x, r), funnel(x.z, x.y, r), funnel(x.w, x.z, r),
                        funnel(y.x, x.w, r));
    case 1:
      return make_uint4(funnel(x.z, x.y, r), funnel(x.w, x.z, r), funnel(y.x, x.w, r),
                        funnel(y.y, y.x, r));
    case 2:
      return make_uint4(funnel(x.w, x.z, r), funnel(y.x, x.w, r), funnel(y.y, y.x, r),
                        funnel(y.z, y.y, r));
    default:
      return make_uint4(funnel(y.x, x.w, r), funnel(y.y, y.x, r), funnel(y.z, y.y, r),
                        funnel(y.w, y.z, r));
  }
}

// The tile pass is a sequence of phases (tile_pass, below), each a function
// of small plain structs.  (The measured alternatives -- other cuts, phase
// probes, per-chunk lookups, direct global loads, omitted output classes --
// are compositions of these phases in okv_decode_ablate.inc, ablation build
// only.)
constexpr uint32_t kLineExt = 512;  // source bytes a tile stages past its end (the line cut's reach)
struct TileBlock {  // the tile's block: uniform (SGPRs)
  uint32_t b, t;    // block, tile of the block
  uint64_t off, row0, kb0, vb0;
  int32_t st;
  uint64_t rows, pend;
};
struct TileExtent {  // the tile: source bytes [P0, P1) of the block, stage lines [A, A + 16 np)
  uint32_t rows, lastr, P0, P1;
  bool last_tile;
  int64_t A;
  uint32_t np;
};
struct TileLane {  // wave 0, lane r = row r: lengths, exclusive prefixes, block positions
  uint32_t k, v, kp, vp, ks, vs;
  bool live;
};
struct TileCuts {  // owned key range [x0, x1), value range [x2, x3) (region bytes)
  uint32_t x[4], KT, VT, jv;  // region totals; jv: the row holding x2
};
struct TileOwned {  // what every wave reads back from the LDS tables
  uint32_t kx0, kx1, vx0, vx1, nunit, nbnd;
};

template <bool kXcd>
__device__ __forceinline__ uint32_t tile_index() {
  if constexpr (kXcd) return (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  return blockIdx.x;
}

// The block's scalars, bases and status, and (wave 0) its record table: one trip.
__device__ __forceinline__ TileBlock tile_block(const CopyParams& P, uint32_t L, uint32_t tpb,
                                                uint32_t& rec, uint32_t& kl) {
  // uniform block index (an SGPR: the loads below are scalar, all in one trip)
  const uint32_t b = __builtin_amdgcn_readfirstlane(L / tpb);
  const uint32_t t = L - b * tpb;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  rec = 0, kl = 0;
  if (tid < 64) {
    rec = P.rt_pos[rec_index(P.nblk, b, lane)];
    kl = P.rt_kl[rec_index(P.nblk, b, lane)];
  }
  const uint64_t off = P.descs[b].offset;
  const BlockCount c = P.cnt[b];
  const Prefix lpre = P.lp[b], tpre = P.tile_pre[b / kTile];
  // consume every scalar here: the scheduler otherwise sinks each load to its
  // first use, one dependent trip after another
  asm volatile("" ::"s"(off), "s"(c.rows), "s"(c.kbytes), "s"(c.vbytes), "s"(c.pend),
               "s"(c.status), "s"(lpre.rows), "s"(lpre.kb), "s"(lpre.vb), "s"(tpre.rows),
               "s"(tpre.kb), "s"(tpre.vb));
  const uint64_t row0 = tpre.rows + lpre.rows, kb0 = tpre.kb + lpre.kb, vb0 = tpre.vb + lpre.vb;
  const bool fits = row0 + c.rows <= P.row_cap &&
                    (P.index_only ||
                     (kb0 + round16(c.kbytes) <= P.key_cap && vb0 + round16(c.vbytes) <= P.val_cap));
  const int32_t st = (c.status == OKV_BLK_OK && !fits) ? int32_t(OKV_BLK_CAPACITY) : c.status;
  return {b, t, off, row0, kb0, vb0, st, c.rows, c.pend};
}

// Tile 0 writes the block outputs and the SoA row index.  Stores wait
// until the LDS tables are built: the compiler makes wave 0's LDS writes
// wait for the wave's outstanding memory operations (it cannot tell them
// from the DMA's LDS target).
__device__ __forceinline__ void block_outputs(const CopyParams& P, const TileBlock& B) {
  if (B.t == 0 && threadIdx.x == 0) {
    P.row_start[B.b] = B.row0;
    if (P.key_base) P.key_base[B.b] = B.kb0;
    if (P.val_base) P.val_base[B.b] = B.vb0;
    P.blk_status[B.b] = B.st;
  }
}

// The early outs: nothing for this tile to copy.
template <uint32_t kT>
__device__ __forceinline__ bool tile_idle(const CopyParams& P, const TileBlock& B) {
  // big blocks are okv_copy_kernel's (the same test as okv_count_kernel's)
  return B.st != OKV_BLK_OK || B.rows == 0 || B.rows > uint64_t(kRCap) || B.pend > P.span_cap ||
         B.pend >= (uint64_t(1) << 32) || B.t * kT >= B.pend;
}

template <uint32_t kT>
__device__ __forceinline__ TileExtent tile_extent(const TileBlock& B) {
  const uint32_t rows = uint32_t(B.rows), P0 = B.t * kT;
  const uint32_t P1 = uint32_t(min<uint64_t>(uint64_t(P0) + kT, B.pend));
  const bool last_tile = P1 == B.pend;
  // stage = segment lines [A, E): the line before the one holding the tile's
  // first byte (a chunk's window begins up to 15 bytes before its first owned
  // byte) through the line after the one holding its last byte + 15, and the
  // line cut's extension
  const int64_t A = int64_t((B.off + P0) & ~uint64_t(15)) - 16;
  const int64_t E = int64_t((B.off + P1 + 15) & ~uint64_t(15)) + 16 + (last_tile ? 0 : kLineExt);
  return {rows, rows - 1, P0, P1, last_tile, A, uint32_t((E - A) >> 4)};
}

// Waves 1.. issue the DMA; wave 0 builds the row table meanwhile.  (With a
// share of the DMA in flight, wave 0's LDS row-table writes would wait for
// it: the compiler cannot tell them apart from the DMA's LDS target.)
template <uint32_t kNT>
__device__ __forceinline__ void tile_dma(const CopyParams& P, const TileBlock& B,
                                         const TileExtent& X, uint4* stage) {
  const uint32_t tid = threadIdx.x;
  if (!P.index_only && tid >= 64) {
    const int64_t lim = int64_t(round16(P.seg_bytes));
    const uint32_t u = tid - 64;
    for (uint32_t k0 = 0; k0 < X.np; k0 += kNT - 64) {
      const uint32_t i = k0 + u;
      if (i < X.np) {
        int64_t a = X.A + (int64_t(i) << 4);
        if (a < 0 || a + 16 > lim) a = int64_t(B.off) & ~int64_t(15);  // bytes never used
        __builtin_amdgcn_global_load_lds(P.seg + a, OKV_LDS_PTR(stage + k0 + (u & ~63u)), 16,
                                         0, 0);
      }
    }
  }
}

// The row table (wave 0, lane r = row r) while the tile is in flight.
template <class Rows>
__device__ __forceinline__ TileLane tile_row_table(const TileBlock& B, const TileExtent& X,
                                                   uint32_t rec, uint32_t kl, Rows& R) {
  const uint32_t lane = threadIdx.x & 63;
  const bool live = lane < X.rows;
  uint32_t nxt = __builtin_amdgcn_update_dpp(0u, rec, 0x130, 0xf, 0xf, false);  // rec[lane + 1]
  if (lane == X.lastr) nxt = uint32_t(B.pend);
  const uint32_t k = live ? kl : 0u, v = live ? nxt - rec - 6 - kl : 0u;
  const uint32_t ki = wave_scan_dpp(k), vi = wave_scan_dpp(v);
  const uint32_t kp = ki - k, vp = vi - v;
  const uint32_t ks = rec + 6, vs = rec + 6 + k;  // block positions of the key / value
  if (live) {
    R.pre[0][lane] = kp;
    R.pre[1][lane] = vp;
    R.sb[0][lane] = ks - kp;
    R.sb[1][lane] = vs - vp;
    if (lane == X.lastr) {
      R.pre[0][X.rows] = ki;
      R.pre[1][X.rows] = vi;
    }
  }
  return {k, v, kp, vp, ks, vs, live};
}

// The first region byte whose source is >= Q (tot when none is).
// (row: the lane holding that byte; lastr when none does)
__device__ __forceinline__ uint32_t first_at(bool live, uint32_t lastr, uint32_t len, uint32_t src,
                                             uint32_t pr, uint32_t tot, uint32_t Q,
                                             uint32_t& row) {
  const uint64_t mk = __ballot(live && len && src + len > Q);
  row = lastr;
  if (!mk) return tot;
  const uint32_t j = uint32_t(__ffsll(static_cast<unsigned long long>(mk)) - 1);
  row = j;
  const uint32_t s0 = __builtin_amdgcn_readlane(src, j), p0 = __builtin_amdgcn_readlane(pr, j);
  return Q > s0 ? p0 + (Q - s0) : p0;
}

// The owned ranges: [first byte whose source is >= P0, same for P1); the
// last tile also owns the 16-byte padding after the region.
__device__ __forceinline__ TileCuts tile_owned_ranges(const TileLane& W, const TileExtent& X) {
  TileCuts C;
  uint32_t jx;
  C.KT = __builtin_amdgcn_readlane(W.kp + W.k, X.lastr);
  C.VT = __builtin_amdgcn_readlane(W.vp + W.v, X.lastr);
  C.x[0] = first_at(W.live, X.lastr, W.k, W.ks, W.kp, C.KT, X.P0, jx);
  C.x[1] = X.last_tile ? uint32_t(round16(C.KT))
                       : first_at(W.live, X.lastr, W.k, W.ks, W.kp, C.KT, X.P1, jx);
  C.x[2] = first_at(W.live, X.lastr, W.v, W.vs, W.vp, C.VT, X.P0, C.jv);
  C.x[3] = X.last_tile ? uint32_t(round16(C.VT))
                       : first_at(W.live, X.lastr, W.v, W.vs, W.vp, C.VT, X.P1, jx);
  return C;
}

// A value cut Y at source Q moves up to the next 128-byte line of the arena
// when the bytes it adds have their sources within kLineExt - 32 of Q
// (the tile before the cut stages that far); both tiles of a cut
// decide from the same row table, so they agree.
__device__ __forceinline__ uint32_t line_cut(const TileLane& W, uint64_t vb0, uint32_t VT,
                                             uint32_t Y, uint32_t Q) {
  const uint32_t end = uint32_t(round16(VT));
  uint32_t Yl = uint32_t(((vb0 + Y + 127) & ~uint64_t(127)) - vb0);
  Yl = Yl > end ? end : Yl;
  if (Yl <= Y || Y >= VT) return Yl <= Y ? Y : Yl;
  const uint32_t y = min(Yl, VT) - 1;  // the last real byte the tile would add
  const uint64_t mk = __ballot(W.live && W.v && W.vp <= y && y < W.vp + W.v);
  if (!mk) return Y;
  const uint32_t j = uint32_t(__ffsll(static_cast<unsigned long long>(mk)) - 1);
  const uint32_t sy = __builtin_amdgcn_readlane(W.vs, j) + (y - __builtin_amdgcn_readlane(W.vp, j));
  return sy + 32 <= Q + kLineExt ? Yl : Y;
}
__device__ __forceinline__ void tile_line_cut(const TileBlock& B, const TileExtent& X,
                                              const TileLane& W, TileCuts& C) {
  if (B.t != 0) C.x[2] = line_cut(W, B.vb0, C.VT, C.x[2], X.P0);
  if (!X.last_tile) C.x[3] = line_cut(W, B.vb0, C.VT, C.x[3], X.P1);
  if (C.x[2] > C.x[3]) C.x[2] = C.x[3];
  // the row holding X2 (head chunk: none when X2 is line-aligned)
  const uint64_t mh = __ballot(W.live && W.v && W.vp <= C.x[2] && C.x[2] < W.vp + W.v);
  C.jv = mh ? uint32_t(__ffsll(static_cast<unsigned long long>(mh)) - 1) : X.lastr;
}

template <class Rows>
__device__ __forceinline__ void tile_put_cuts(const TileCuts& C, Rows& R) {
  if ((threadIdx.x & 63) == 0) {
    R.x[0] = C.x[0];
    R.x[1] = C.x[1];
    R.x[2] = C.x[2];
    R.x[3] = C.x[3];
  }
}
// Granule table of a range [X0, X1) of a region: gt[g - (X0 >> 6)] = row
// holding byte max(64 g, X0); granules past the last row's bytes (padding)
// keep the preset lastr.  The product builds the key range's only: the
// values' boundary chunks carry their row.  (pr, ln: the lane's prefix and
// length in the region.)
__device__ __forceinline__ void tile_granules(const TileExtent& X, bool live, uint32_t pr,
                                              uint32_t ln, uint32_t X0, uint32_t X1, uint8_t* gt) {
  const uint32_t lane = threadIdx.x & 63;
  if (X1 <= X0) return;
  const uint32_t g0 = X0 >> 6, gl = (X1 - 1) >> 6;
  for (uint32_t g = g0 + lane; g <= gl; g += 64) gt[g - g0] = uint8_t(X.lastr);
  if (live && ln) {
    const uint32_t e = pr + ln;
    if (pr <= X0 && X0 < e) gt[0] = uint8_t(lane);
    const uint32_t gs = max(g0 + 1, (pr + 63) >> 6), ge = min(gl, ((e + 63) >> 6) - 1);
    for (uint32_t g = gs; g <= ge; ++g) gt[g - g0] = uint8_t(lane);
  }
}

// The value units and boundary chunks of the owned value range.
template <class Rows>
__device__ __forceinline__ void tile_value_units(const TileBlock& B, const TileExtent& X,
                                                 const TileLane& W, const TileCuts& C, Rows& R) {
  const uint32_t lane = threadIdx.x & 63;
  // row pieces of the owned value range: [a, e) = row r's bytes in [X2, X3)
  const uint32_t X2 = C.x[2], X3 = C.x[3];
  const uint32_t a = max(W.vp, X2), e = min(W.vp + W.v, X3);
  const bool piece = W.live && W.v && a < e;
  const uint32_t cs = piece ? (a + 15) >> 4 : 0u, ce = piece ? e >> 4 : 0u;
  const uint32_t wc = ce > cs ? ce - cs : 0u;
  const uint32_t nu = (wc + 63) >> 6;
  const uint32_t ui = wave_scan_dpp(nu);
  const uint32_t sbias0 = uint32_t(int64_t(B.off) - X.A);
  for (uint32_t q = 0; q < nu; ++q) {
    const uint32_t u = ui - nu + q;
    R.unit[0][u] = cs + 64 * q;
    R.unit[1][u] = W.vs - W.vp + 16 * (cs + 64 * q) + sbias0;
    R.unit[2][u] = min(64u, wc - 64 * q);
  }
  // boundary chunks: where a piece ends inside a chunk, and the range's
  // first chunk when it starts inside one (in order; equal neighbours
  // skipped), as chunk << 8 | the row holding the chunk's first owned
  // byte: the lowest row whose piece ends in the chunk (a row before it
  // holding that byte would end in the chunk too), or for the head chunk
  // the row holding X2
  const bool eb = piece && (e & 15);
  const uint64_t m = __ballot(eb);
  const uint32_t head = (X2 < X3 && (X2 & 15)) ? 1u : 0u;
  const uint32_t idx = head + uint32_t(__builtin_amdgcn_mbcnt_hi(
                                  uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u)));
  if (eb) R.bnd[idx] = ((e >> 4) << 8) | lane;
  // read lane 63 with the whole wave active (inside the lane-0 branch the
  // compiler may compute ui for lane 0 only)
  const uint32_t nunit = __builtin_amdgcn_readlane(ui, 63);
  if (lane == 0) {
    if (head) R.bnd[0] = ((X2 >> 4) << 8) | C.jv;
    R.nbnd = head + uint32_t(__builtin_popcountll(m));
    R.nunit = nunit;
  }
}

// Index-only decodes: tile 0 writes the SoA row index (spans into seg).
__device__ __forceinline__ void tile_index_rows(const CopyParams& P, const TileBlock& B,
                                                const TileLane& W) {
  if (P.index_only && B.t == 0 && W.live) {
    const uint64_t g = B.row0 + (threadIdx.x & 63);
    P.key_len[g] = uint16_t(W.k);
    P.val_len[g] = W.v;
    P.key_off[g] = B.off + W.ks;
    P.val_off[g] = B.off + W.vs;
  }
}

// The DMA waves wait for their loads (wave 0 has none: its SoA stores drain
// on their own); then the tables and the stage are everyone's.
__device__ __forceinline__ void tile_wait_stage() {
  if (threadIdx.x >= 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// Tile 0: the block outputs and the SoA row index (from the LDS tables).
template <class Rows>
__device__ __forceinline__ void tile_row_index(const CopyParams& P, const TileBlock& B,
                                               const TileExtent& X, const Rows& R) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  if (B.t == 0 && tid < 64) {
    block_outputs(P, B);
    if (lane < X.rows) {
      const uint64_t g = B.row0 + lane;
      const uint32_t kp = R.pre[0][lane], vp = R.pre[1][lane];
      P.key_len[g] = uint16_t(R.pre[0][lane + 1] - kp);
      P.val_len[g] = R.pre[1][lane + 1] - vp;
      P.key_off[g] = B.kb0 + kp;
      P.val_off[g] = B.vb0 + vp;
    }
  }
}

// The ranges and counts wave 0 left in LDS (read together: one trip).
template <class Rows>
__device__ __forceinline__ TileOwned tile_owned(const Rows& R) {
  return {R.x[0], R.x[1], R.x[2], R.x[3], R.nunit, R.nbnd};
}

// Value runs: one unit of <= 64 whole chunks of one row per wave iteration.
template <uint32_t kNT, class Rows>
__device__ __forceinline__ void tile_store_runs(const CopyParams& P, const TileBlock& B,
                                                const Rows& R, const uint4* stage,
                                                uint32_t nunit) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  uint8_t* const varena = P.val_arena + B.vb0;
  for (uint32_t u = tid >> 6; u < nunit; u += kNT / 64) {
    const uint32_t c0 = __builtin_amdgcn_readfirstlane(R.unit[0][u]);
    const uint32_t sbyte = __builtin_amdgcn_readfirstlane(R.unit[1][u]);
    const uint32_t cnt = __builtin_amdgcn_readfirstlane(R.unit[2][u]);
    if (lane < cnt) {
      const uint32_t line = (sbyte >> 4) + lane;
      const uint4 w = funnel_u(stage[line], stage[line + 1], sbyte & 15);
      *reinterpret_cast<uint4*>(varena + (uint64_t(c0 + lane) << 4)) = w;
    }
  }
}
// Bytes [lo, hi) of the region's chunk [x, x + 16), row by row from row r on
// (zero past the region): src(s) = the 16 bytes at block position s.
template <class Src>
__device__ __forceinline__ uint4 chunk_bytes(const uint32_t* pre, const uint32_t* sb,
                                             uint32_t rows, uint32_t r, uint32_t x, uint32_t lo,
                                             uint32_t hi, Src src) {
  const uint32_t dend = min(hi, pre[rows]);
  uint4 out = make_uint4(0, 0, 0, 0);
  for (uint32_t d = lo; d < dend; ++r) {
    const uint32_t e = min(dend, pre[r + 1]);
    if (e > d) {  // bytes [d, e) of the chunk from row r
      out = merge_bytes(out, src(sb[r] + x), int32_t(d - x), int32_t(e - x));
      d = e;
    }
  }
  return out;
}

// Chunk j of the keys (j < nk) and the boundary value chunks, by per-lane
// lookup: its 16 bytes at dst, of which [lo, hi) are the tile's.  False for a
// boundary chunk equal to its neighbour (nothing to store).
struct TileChunk {
  uint8_t* dst;
  uint4 out;
  uint32_t lo, hi;
};
template <class Rows>
__device__ __forceinline__ bool tile_chunk(const CopyParams& P, const TileBlock& B,
                                           const TileExtent& X, const Rows& R, const uint8_t* gt,
                                           const uint4* stage, const TileOwned& O, uint32_t nk,
                                           uint32_t j, TileChunk& c) {
  const uint32_t sbias = uint32_t(int64_t(B.off) - X.A);  // stage byte of block position s: s + sbias
  const uint32_t reg = j >= nk;
  const uint32_t bv = reg ? R.bnd[j - nk] : 0u;
  if (reg && j > nk && (bv >> 8) == (R.bnd[j - nk - 1] >> 8)) return false;
  const uint32_t X0 = reg ? O.vx0 : O.kx0, X1 = reg ? O.vx1 : O.kx1;
  const uint32_t x = reg ? (bv >> 8) << 4 : ((O.kx0 >> 4) + j) << 4;
  const uint32_t lo = max(x, X0), hi = min(x + 16, X1);
  const uint32_t* pre = R.pre[reg];
  const uint32_t* sb = R.sb[reg];
  uint32_t r = reg ? (bv & 255u) : uint32_t(gt[(lo >> 6) - (X0 >> 6)]);
  while (r < X.lastr && pre[r + 1] <= lo) ++r;
  c.dst = (reg ? P.val_arena + B.vb0 : P.key_arena + B.kb0) + x;
  c.out = chunk_bytes(pre, sb, X.rows, r, x, lo, hi,
                      [&](uint32_t s) { return load16_lds_b128(stage, s + sbias); });
  c.lo = lo - x;
  c.hi = hi - x;
  return true;
}

// Keys and the boundary value chunks.  A whole chunk is one 16-byte store; a
// chunk the neighbouring tile shares is stored byte-exactly (disjoint bytes).
template <uint32_t kNT, class Rows>
__device__ __forceinline__ void tile_store_chunks(const CopyParams& P, const TileBlock& B,
                                                  const TileExtent& X, const Rows& R,
                                                  const uint8_t* gt, const uint4* stage,
                                                  const TileOwned& O) {
  const uint32_t nk = O.kx1 > O.kx0 ? ((O.kx1 + 15) >> 4) - (O.kx0 >> 4) : 0u;
  for (uint32_t j = threadIdx.x; j < nk + O.nbnd; j += kNT) {
    TileChunk c;
    if (!tile_chunk(P, B, X, R, gt, stage, O, nk, j, c)) continue;
    if (c.lo == 0 && c.hi == 16)
      *reinterpret_cast<uint4*>(c.dst) = c.out;
    else
      store_partial(c.dst, c.out, c.lo, c.hi);
  }
}

// The product form: the phases in order.
template <uint32_t kT, uint32_t kNT, bool kXcd>
__device__ __forceinline__ void tile_pass(const CopyParams& P, uint32_t tpb, uint32_t ntile) {
  __shared__ TileRows<kT> R;
  __shared__ uint8_t gt[kT / 64 + 8];  // row holding key byte max(64 g, range start), per 64-byte granule
  __shared__ uint4 stage[(kT + kLineExt) / 16 + 4];
  const uint32_t L = tile_index<kXcd>();
  if (L >= ntile) return;
  uint32_t rec, kl;
  const TileBlock B = tile_block(P, L, tpb, rec, kl);
  if (tile_idle<kT>(P, B)) {
    block_outputs(P, B);
    return;
  }
  const TileExtent X = tile_extent<kT>(B);
  tile_dma<kNT>(P, B, X, stage);
  if (threadIdx.x < 64) {
    const TileLane W = tile_row_table(B, X, rec, kl, R);
    if (!P.index_only) {
      TileCuts C = tile_owned_ranges(W, X);
      tile_line_cut(B, X, W, C);
      tile_put_cuts(C, R);
      tile_granules(X, W.live, W.kp, W.k, C.x[0], C.x[1], gt);
      tile_value_units(B, X, W, C, R);
    }
    tile_index_rows(P, B, W);
  }
  if (P.index_only) {
    block_outputs(P, B);
    return;
  }
  tile_wait_stage();
  tile_row_index(P, B, X, R);
  const TileOwned O = tile_owned(R);
  tile_store_runs<kNT>(P, B, R, stage, O.nunit);
  tile_store_chunks<kNT>(P, B, X, R, gt, stage, O);
}

// 8 waves per SIMD (8 workgroups per CU: the LDS bound; registers capped at
// 64 per lane, no spills; the uncapped form measured equal).
template <uint32_t kT, uint32_t kNT, bool kXcd>
__global__ __launch_bounds__(kNT) __attribute__((amdgpu_waves_per_eu(kT <= 16384 || kNT == 1024 ? 8 : 4))) void okv_tile_kernel(
    CopyParams P, uint32_t tpb, uint32_t ntile) {
  tile_pass<kT, kNT, kXcd>(P, tpb, ntile);
}

#ifdef OKV_ABLATE  // the measured alternative pass-3 forms (ablation build only)
#include "okv_decode_ablate.inc"
#endif


// Pass 3, small-block staged form (blocks averaging <= 16 KiB, e.g. 4 KiB
// blocks): one wave per block DMAs the whole block into its LDS stage right
// after the metadata arrives, then reads the record headers and assembles
// every key and value chunk from the stage: two dependent HBM trips per block
// (metadata + record positions, then the block) instead of four (metadata,
// positions, headers, key tiles, value tiles).  Blocks that do not fit the
// stage take the global-window gather (same workgroup, same row table code).
constexpr uint32_t kSmallStage = 5 * 1024;  // staged bytes per block (DMA pieces of 1 KiB)

__global__ __launch_bounds__(64) void okv_gather_small_kernel(CopyParams P) {
  __shared__ GatherSmem sm;
  __shared__ uint4 stage[kSmallStage / 16 + 4];
  const uint32_t lane = threadIdx.x;
  for (uint32_t b = blockIdx.x; b < P.nblk; b += gridDim.x) {
    // record positions ride with the metadata (slots exist for every r < kRCap)
    const uint32_t rec0 = P.rt_pos[rec_index(P.nblk, b, lane)];
    const BlockMeta m = block_meta(P, b);
    if (block_head(P, b, m)) {
      const int rows = int(m.c.rows);
      const uint32_t rec = int(lane) < rows ? rec0 : 0u;
      const uint32_t shift = uint32_t(m.off & 15);
      // stage byte 0 = block byte -(16 + shift): a 16-byte lead-in for
      // windows that begin before a row, and 32 bytes of slack at the end
      const uint32_t need = 16 + shift + uint32_t(m.c.pend) + 32;
      if (need <= kSmallStage && !P.index_only) {
        const Staged src{stage, stage_block_wave(stage, P.seg, P.seg_bytes, m.off,
                                                 uint32_t(m.c.pend), lane)};
        build_row_table(src, sm, rows, rec);
        write_row_index(P, sm, m, rows);
        gather_region<false>(src, sm, rows, P.key_arena, m.B.kb0, 0, 1);
        gather_region<true>(src, sm, rows, P.val_arena, m.B.vb0, 0, 1);
      } else {
        const GlobalWin src{P.seg, P.seg_bytes, m.off};
        build_row_table(src, sm, rows, rec);
        write_row_index(P, sm, m, rows);
        if (!P.index_only) {
          gather_region<false>(src, sm, rows, P.key_arena, m.B.kb0, 0, 1);
          gather_region<true>(src, sm, rows, P.val_arena, m.B.vb0, 0, 1);
        }
      }
    }
  }
}

// Single-pass decode for small batches of small blocks (<= kFusedMaxBlocks
// blocks averaging <= 16 KiB): passes 1-3 in ONE launch.  One wave per block,
// the block index from blockIdx.x: it DMAs the whole block into LDS, walks its
// record headers there as the Go loop does (walk_staged_to; statuses as in
// okv_count_kernel) and publishes the block's counts with the call's epoch
// tag in one packed 8-byte look-back word (fused_pack; counts that do not fit
// go through F.agg[b]).  Its exclusive prefix is the sum of the words of all
// the blocks before it, every lane polling up to kFusedMaxBlocks / 64 of
// them; then it gathers its rows from its stage.  No arrival counter, no scan
// by the last arrival, and -- the tag making every call's words fresh -- no
// reset between calls.  Blocks with more than kRCap rows, or too large to
// stage, get their counts the same way (a global-memory walk) and go to
// okv_copy_kernel through the big-block list, with cnt / lp / tile_pre
// written as passes 1-2 would.
// Precondition (kept by okv_open's fused_max): the whole grid is resident at
// once and dispatched in index order.  A block spins on the words of lower
// indices only, which is safe only if those blocks have started: a grid past
// the device's resident capacity, or dispatched out of order, could leave the
// resident blocks spinning on ones that never start.
constexpr uint32_t kFusedMaxBlocks = 512;
struct FusedParams {
  const int32_t* pre;     // zstd-stage statuses or null
  BlockCount* cnt;        // what passes 1-2 write, for okv_copy_kernel
  Prefix* lp;
  Prefix* tile_pre;
  uint32_t* flag;         // [nblk] 8-byte look-back words (fused_pack); the stream arm's flags:
                          // (epoch << 2) | 1 aggregate, | 2 inclusive
  Prefix* agg;            // [nblk]
  Prefix* incl;           // [nblk]
  // (the stream and block arms of the ablation build only; the fused kernel reads none)
  unsigned long long* ctr;  // block-index counter (monotone across calls)
  unsigned long long* arr;  // arrival counter (monotone across calls, same base)
  unsigned long long base;  // its value at this call's start
  uint32_t epoch;
  Totals* tot;
  uint32_t* big_zero;  // the other big-block counter slot: zeroed for the next launch
};

// Hand-off without release/acquire fences (an agent-scope release writes back
// the whole L2, an acquire invalidates it -- per block, that swamps the
// kernel): payload and flag go through coherent (sc1) stores, the payload
// drained before the flag, and the reader polls and reads with sc1 loads
// (cdna_hip_programming.md G16, valid forms).
__device__ __forceinline__ void publish(uint32_t* f, Prefix* slot, const Prefix& v, uint32_t tag) {
  __hip_atomic_store(&slot->rows, v.rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&slot->kb, v.kb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&slot->vb, v.vb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&slot->bad, v.bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(f, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void publish_payload(Prefix* slot, const Prefix& v) {
  __hip_atomic_store(&slot->rows, v.rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&slot->kb, v.kb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&slot->vb, v.vb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&slot->bad, v.bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ uint32_t flag_peek(const uint32_t* f) {
  return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ Prefix prefix_peek(const Prefix* slot) {
  Prefix v;
  v.rows = __hip_atomic_load(&slot->rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  v.kb = __hip_atomic_load(&slot->kb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  v.vb = __hip_atomic_load(&slot->vb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  v.bad = __hip_atomic_load(&slot->bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// fused_pass<kLB = true> is the ablation build's stream kernel
// (okv_decode_ablate_lb.inc), for batches of any size: block indices by
// arrival and the exclusive prefix by this decoupled look-back, so no block
// waits for one that may not be resident.  Declared here, defined only there;
// the product kernel is fused_pass<false>, which never calls it.
__device__ Prefix fused_prefix_lookback(const CopyParams& P, const FusedParams& F, uint32_t b,
                                        uint32_t lane, uint32_t tag, const Prefix& mine);
#ifdef OKV_ABLATE
// (ablation build: wall-clock stamps of the fused kernel's phases per block --
// start, staged, walked, prefix known, done; okv_debug_fused_times)
__device__ uint64_t g_fused_t[kFusedMaxBlocks * 8];
#define OKV_FUSED_STAMP(i) \
  if (lane == 0 && b < kFusedMaxBlocks) g_fused_t[b * 8 + (i)] = wall_clock64()
#else
#define OKV_FUSED_STAMP(i)
#endif

// The fused kernel's look-back word per block: (epoch | 1 << 31) << 32 | its
// counts packed in 30 bits -- rows (10), padded key bytes / 16 (9), padded
// value bytes / 16 (9), failed (1), overflow (1: the counts do not fit and
// are in F.agg[b], published before the word).  One 8-byte write-through
// store is the payload and the flag at once.
__device__ __forceinline__ bool fused_pack(const Prefix& v, uint32_t& w) {
  if (v.rows >= 1024 || v.kb >= (512u << 4) || v.vb >= (512u << 4)) return false;
  w = uint32_t(v.rows) | uint32_t(v.kb >> 4) << 10 | uint32_t(v.vb >> 4) << 19 |
      uint32_t(v.bad) << 28;
  return true;
}

// A small block's header walk from its LDS stage is walk_staged_to (okv_kernels.hpp;
// C2's fixed 86-byte records: all 42 in one round), record positions of rows < kRCap
// going to rec[] (RecSink).  The same walk in HBM by lane 0 (a block too large for the
// stage); the results are broadcast to the wave.
__device__ __forceinline__ void walk_global(const uint8_t* seg, uint64_t off, uint64_t len,
                                            uint64_t original_size, uint32_t* rec, uint32_t lane,
                                            int32_t& st, uint64_t& rows, uint64_t& kb,
                                            uint64_t& vb, uint64_t& p) {
  rows = kb = vb = p = 0;
  if (lane == 0) {
    const uint64_t orig = go_walk_bound(original_size);
    while (p < orig) {  // :340
      if (len - p < 6) { st = OKV_BLK_PANIC; break; }  // :342-345
      uint32_t kl, vl;
      header_global(seg, off + p, kl, vl);
      const uint64_t room = len - p - 6;
      if (kl > room || vl > room - kl) { st = OKV_BLK_PANIC; break; }  // :346-349
      if (rows < kRCap) rec[rows] = uint32_t(p);
      rows++;
      kb += kl;
      vb += vl;
      p += 6 + uint64_t(kl) + uint64_t(vl);
    }
    if (st != OKV_BLK_OK) rows = kb = vb = 0;
  }
  st = __shfl(st, 0, 64);
  rows = __shfl(rows, 0, 64);
  kb = __shfl(kb, 0, 64);
  vb = __shfl(vb, 0, 64);
  p = __shfl(p, 0, 64);
}

template <bool kLB>  // (kLB: the ablation build's stream kernel only)
__device__ __forceinline__ void fused_pass(const CopyParams& P, const FusedParams& F) {
  __shared__ GatherSmem sm;
  __shared__ uint4 stage[kSmallStage / 16 + 4];
  const uint32_t lane = threadIdx.x;
  uint32_t b = blockIdx.x;
  if constexpr (kLB) {  // blocks by arrival (the stream kernel's grid is not resident)
    __shared__ uint32_t s_b;
    if (lane == 0) s_b = uint32_t(atomicAdd(F.ctr, 1ull) - F.base);
    __syncthreads();
    b = s_b;
    if (b >= P.nblk) return;
  }
  // (the product grid is all resident -- a quarter of the device's capacity
  // -- and dispatched in index order, so a block waits only on lower indices
  // that have started: no block-index counter)
  const uint32_t tag = F.epoch << 2;
  OKV_FUSED_STAMP(0);
  if (b == 0 && lane == 0) *F.big_zero = 0;
  // ---- pass 1 for this block (okv_count_kernel's rules) ----
  const Desc d = P.descs[b];
  uint64_t len;
  int32_t st = entry_status(d, P.seg_bytes, P.comp, F.pre, b, len);
  const uint32_t shift = uint32_t(d.offset & 15);
  const bool staged = st == OKV_BLK_OK && len + 16 + shift + 32 <= kSmallStage;
  if (staged && len)  // the whole block (BlockSize bytes) into the stage
    stage_block_wave<kSmallStage>(stage, P.seg, P.seg_bytes, d.offset, uint32_t(len), lane);
  __syncthreads();
  OKV_FUSED_STAMP(1);
  const Staged lsrc{stage, 16 + shift};
  uint64_t rows = 0, kb = 0, vb = 0, p = 0;
  if (st == OKV_BLK_OK && staged)
    walk_staged_to(lsrc, uint32_t(len), d.original_size, RecSink{sm.rec, kRCap}, lane, st, rows,
                   kb, vb, p);
  else if (st == OKV_BLK_OK)  // not stageable: lane 0 walks the headers in HBM
    walk_global(P.seg, d.offset, len, d.original_size, sm.rec, lane, st, rows, kb, vb, p);
  __syncthreads();  // the walk's record positions (sm.rec) are read by every lane below
  OKV_FUSED_STAMP(2);
  const Prefix mine{rows, round16(kb), round16(vb), uint64_t(st != OKV_BLK_OK)};
  Prefix ex{0, 0, 0, 0};
  // ---- pass 2: each block sums its predecessors' published counts ----
  // One write-through 8-byte word per block carries its counts and the
  // call's tag (fused_pack); every lane loads the words of up to
  // kFusedMaxBlocks / 64 predecessors at once and re-polls only those not
  // yet published.  (Round 5: the last block to arrive scanned every
  // block's counts and published the prefixes behind a second flag -- a
  // chain of dependent cross-XCD trips that every block waited out.)
  uint64_t* word = reinterpret_cast<uint64_t*>(F.flag);
  const uint32_t want = F.epoch | 0x80000000u;
  if (!kLB && lane == 0) {
    uint32_t w = 0;
    if (!fused_pack(mine, w)) {
      publish_payload(&F.agg[b], mine);  // sc1 stores, drained
      w = 1u << 29;
    }
    __hip_atomic_store(&word[b], uint64_t(want) << 32 | w, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  // Pass 3 up to the stores, while the predecessors' counts arrive: a staged
  // block's key and value regions are assembled into an LDS image (block-
  // local offsets); only the row index and the image's copy-out wait for the
  // prefix.  (C2: the gather after the wait took 3.0 us of a 14 us kernel.)
  __shared__ uint4 img[kSmallStage / 16 + 2];
  const int nr = int(rows);
  const bool pre_asm = !kLB && staged && st == OKV_BLK_OK && nr > 0 && rows <= uint64_t(kRCap) &&
                       !P.index_only;
  const uint32_t kreg = uint32_t(round16(kb)), vreg = uint32_t(round16(vb));
  if (pre_asm) {
    static_assert(sizeof(img) >= kSmallStage, "both regions fit the image");
    const uint32_t rec = int(lane) < nr ? sm.rec[lane] : 0u;
    build_row_table(lsrc, sm, nr, rec);
    uint8_t* const im = reinterpret_cast<uint8_t*>(img);
    gather_region<false>(lsrc, sm, nr, im, 0, 0, 1);
    gather_region<true>(lsrc, sm, nr, im, kreg, 0, 1);
  }
  if constexpr (kLB) {
    ex = fused_prefix_lookback(P, F, b, lane, tag, mine);  // ablation build only
  } else {
    constexpr uint32_t kU = kFusedMaxBlocks / 64;
    uint64_t wv[kU];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint32_t k = lane + 64 * u;
      wv[u] = k < b ? __hip_atomic_load(&word[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                    : uint64_t(want) << 32;
    }
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint32_t k = lane + 64 * u;
      while (uint32_t(wv[u] >> 32) != want) {
        __builtin_amdgcn_s_sleep(1);
        wv[u] = __hip_atomic_load(&word[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const uint32_t w = uint32_t(wv[u]);
      if (w >> 29 & 1u) {
        const Prefix o = prefix_peek(&F.agg[k]);
        ex.rows += o.rows;
        ex.kb += o.kb;
        ex.vb += o.vb;
        ex.bad += o.bad;
      } else {
        ex.rows += w & 1023u;
        ex.kb += uint64_t(w >> 10 & 511u) << 4;
        ex.vb += uint64_t(w >> 19 & 511u) << 4;
        ex.bad += w >> 28 & 1u;
      }
    }
    ex.rows = wave_sum64(ex.rows);
    ex.kb = wave_sum64(ex.kb);
    ex.vb = wave_sum64(ex.vb);
    ex.bad = wave_sum64(ex.bad);
    if (b == P.nblk - 1 && lane == 0) {  // the totals
      *F.tot = Totals{ex.rows + mine.rows, ex.kb + mine.kb, ex.vb + mine.vb, ex.bad + mine.bad};
      P.row_start[P.nblk] = ex.rows + mine.rows;
    }
  }
  OKV_FUSED_STAMP(3);
  // ---- what passes 1-2 leave for okv_copy_kernel, and the totals ----
  if (lane == 0) {
    BlockCount c;
    c.rows = rows;
    c.kbytes = kb;
    c.vbytes = vb;
    c.pend = p;
    c.status = st;
    c.pad = 0;
    F.cnt[b] = c;
    F.lp[b] = ex;
    if (b % kTile == 0) F.tile_pre[b / kTile] = Prefix{0, 0, 0, 0};
    if (st == OKV_BLK_OK && (rows > kRCap || p >= (uint64_t(1) << 32)))
      P.big_list[atomicAdd(P.big_count, 1u)] = b;
  }
  // ---- pass 3 ----
  BlockMeta m;
  m.c = BlockCount{rows, kb, vb, p, st, 0};
  m.B = block_base_of(P, m.c, ex, Prefix{0, 0, 0, 0});
  m.off = d.offset;
  if (!block_head(P, b, m)) {
    OKV_FUSED_STAMP(4);
    return;
  }
  if (pre_asm) {  // the row index, then the image out in whole 16-byte chunks
    write_row_index(P, sm, m, nr);
    for (uint32_t c = lane; c < kreg / 16; c += 64)
      *reinterpret_cast<uint4*>(P.key_arena + m.B.kb0 + 16ull * c) = img[c];
    for (uint32_t c = lane; c < vreg / 16; c += 64)
      *reinterpret_cast<uint4*>(P.val_arena + m.B.vb0 + 16ull * c) = img[kreg / 16 + c];
    OKV_FUSED_STAMP(4);
    return;
  }
  const uint32_t rec = int(lane) < nr ? sm.rec[lane] : 0u;
  if (staged) {
    build_row_table(lsrc, sm, nr, rec);
    write_row_index(P, sm, m, nr);
    if (!P.index_only) {
      gather_region<false>(lsrc, sm, nr, P.key_arena, m.B.kb0, 0, 1);
      gather_region<true>(lsrc, sm, nr, P.val_arena, m.B.vb0, 0, 1);
    }
  } else {
    const GlobalWin gsrc{P.seg, P.seg_bytes, m.off};
    build_row_table(gsrc, sm, nr, rec);
    write_row_index(P, sm, m, nr);
    if (!P.index_only) {
      gather_region<false>(gsrc, sm, nr, P.key_arena, m.B.kb0, 0, 1);
      gather_region<true>(gsrc, sm, nr, P.val_arena, m.B.vb0, 0, 1);
    }
  }
  OKV_FUSED_STAMP(4);
}

__global__ __launch_bounds__(64) void okv_decode_fused_kernel(CopyParams P, FusedParams F) {
  fused_pass<false>(P, F);
}

// ---------------------------------------------------------------------------
// Pass 4 (big blocks only): LDS-staged decode with a serial header chase.
// ---------------------------------------------------------------------------
struct SlowRows {               // general path: 64-bit positions, batched rows
  uint64_t rec[kRowBatch];        // record position within the block
  uint64_t kpre[kRowBatch + 1];   // key-byte prefix within the block
  uint64_t vpre[kRowBatch + 1];   // value-byte prefix within the block
  uint32_t klen[kRowBatch];
  uint32_t vlen[kRowBatch];
};
struct FastRows {               // fast path: block staged in LDS, <= kFastRows rows
  uint32_t rec[kFastRows + 1];    // record position; rec[rows] = end of the walk
  uint32_t kpre[kFastRows + 1];   // exclusive prefix of key lengths
  uint32_t vpre[kFastRows + 1];   // exclusive prefix of value lengths
};
// okv_point_get's probe key (<= 8 KiB): over the fast row table's prefix
// arrays, which its search does not use (the record positions stay live).
struct FindRows {
  uint32_t rec[kFastRows + 1];
  uint32_t key[8192 / 4];
};
static_assert(offsetof(FindRows, key) == offsetof(FastRows, kpre), "key starts at kpre");
static_assert(sizeof(FindRows) <= sizeof(FastRows), "the key adds no LDS");
struct __align__(16) CopySmem {
  uint4 stage[(kStage + kStagePad) / 16];  // [16 B guard][block image][guard]
  union {
    SlowRows s;
    FastRows f;
    FindRows k;
  };
};

// Byte source: the block in HBM (blocks too large to stage).
struct GlobalSrc {
  const uint8_t* seg;
  uint64_t seg_bytes;
  uint64_t off;
  __device__ __forceinline__ void header(uint64_t pos, uint32_t& kl, uint32_t& vl) const {
    header_global(seg, off + pos, kl, vl);
  }
  __device__ __forceinline__ uint4 load16(int64_t pos) const {
    return load16_global(seg, seg_bytes, int64_t(off) + pos);
  }
};


// Copy rows [0, nb) of one region (keys or values) into `arena`:
//   row i bytes = src[spos_i, spos_i + len_i) -> arena[dbase + pre_i, ...).
// Lane groups of G lanes own one row; each lane writes 16-byte aligned
// destination chunks (dwordx4), masked head/tail chunks with narrow stores.
template <class Src>
__device__ __forceinline__ void copy_region(const Src& src, uint8_t* __restrict__ arena,
                                            uint64_t dbase, const uint64_t* pre,
                                            const uint64_t* rec, const uint32_t* klen,
                                            const uint32_t* len, bool is_val, int nb,
                                            uint32_t G) {
  const uint32_t tid = threadIdx.x;
  const uint32_t grp = tid / G, sub = tid % G, ngrp = blockDim.x / G;
  for (uint32_t i = grp; i < uint32_t(nb); i += ngrp) {
    const uint64_t L = len[i];
    if (L == 0) continue;
    const uint64_t d0 = dbase + pre[i];
    const int64_t s0 = int64_t(rec[i] + 6 + (is_val ? klen[i] : 0));
    const uint64_t c0 = d0 & ~uint64_t(15), c1 = (d0 + L + 15) & ~uint64_t(15);
    for (uint64_t ca = c0 + 16ull * sub; ca < c1; ca += 16ull * G) {
      const int64_t rel = int64_t(ca) - int64_t(d0);
      const uint4 v = src.load16(s0 + rel);
      const uint32_t lo = ca < d0 ? uint32_t(d0 - ca) : 0u;
      const uint64_t end = d0 + L - ca;
      const uint32_t hi = end < 16 ? uint32_t(end) : 16u;
      if (lo == 0 && hi == 16) {
        *reinterpret_cast<uint4*>(arena + ca) = v;
      } else {
        store_partial(arena + ca, v, lo, hi);
      }
    }
  }
}

template <class Src>
__device__ __forceinline__ void materialise(const Src& src, const CopyParams& P,
                                           CopySmem& sm, uint64_t rows, uint64_t kbytes,
                                           uint64_t vbytes, uint64_t row0, uint64_t kb0,
                                           uint64_t vb0, uint64_t pend) {
  const uint32_t tid = threadIdx.x;
  const uint32_t Gk = group_size(kbytes / rows), Gv = group_size(vbytes / rows);
  uint64_t p = 0, kacc = 0, vacc = 0;  // chase state (lane 0)
  for (uint64_t r0 = 0; r0 < rows; r0 += kRowBatch) {
    const int nb = int(rows - r0 < kRowBatch ? rows - r0 : kRowBatch);
    if (tid == 0) {
      // serial header chase: record i+1 starts at rec_i + 6 + klen_i + vlen_i
      // (lengths and positions clamped to pass 1's totals and walk end: if the
      // segment changed under the decode, reads stay inside the block's walk
      // and writes inside its regions)
      for (int i = 0; i < nb; ++i) {
        uint32_t kl, vl;
        src.header(p, kl, vl);
        kl = uint32_t(min<uint64_t>(kl, kbytes - kacc));
        vl = uint32_t(min<uint64_t>(vl, vbytes - vacc));
        sm.s.rec[i] = p;
        sm.s.klen[i] = kl;
        sm.s.vlen[i] = vl;
        sm.s.kpre[i] = kacc;
        sm.s.vpre[i] = vacc;
        kacc += kl;
        vacc += vl;
        p = min<uint64_t>(p + 6 + uint64_t(kl) + uint64_t(vl), pend - 6);
      }
      sm.s.kpre[nb] = kacc;
      sm.s.vpre[nb] = vacc;
    }
    __syncthreads();
    // SoA row index (coalesced over rows)
    for (int i = tid; i < nb; i += blockDim.x) {
      const uint64_t g = row0 + r0 + i;
      P.key_off[g] = kb0 + sm.s.kpre[i];
      P.key_len[g] = uint16_t(sm.s.klen[i]);
      P.val_off[g] = vb0 + sm.s.vpre[i];
      P.val_len[g] = sm.s.vlen[i];
    }
    copy_region(src, P.key_arena, kb0, sm.s.kpre, sm.s.rec, sm.s.klen, sm.s.klen, false, nb, Gk);
    copy_region(src, P.val_arena, vb0, sm.s.vpre, sm.s.rec, sm.s.klen, sm.s.vlen, true, nb, Gv);
    __syncthreads();
  }
  // zero the 16-byte padding tail of each arena region
  if (tid == 0) {
    const uint64_t ke = kb0 + kbytes, ve = vb0 + vbytes;
    const uint4 z = make_uint4(0, 0, 0, 0);
    if (ke & 15) store_partial(P.key_arena + (ke & ~uint64_t(15)), z, uint32_t(ke & 15), 16);
    if (ve & 15) store_partial(P.val_arena + (ve & ~uint64_t(15)), z, uint32_t(ve & 15), 16);
  }
}

// ---- fast path: the block is staged in LDS and has <= kFastRows rows ------
// Every arena store is a full, aligned 16-byte chunk.  A chunk is owned by
// the row containing its first byte; its owner lane assembles it in
// registers, merging bytes of the following rows when the chunk spills past
// its row (no partial stores, so neighbouring chunks never race).  The last
// chunk of a region is zero-filled past the region end (16-byte padding).
template <bool kVal>
__device__ __forceinline__ void copy_region_fast(const uint4* __restrict__ s4, uint32_t bias,
                                                 uint8_t* __restrict__ arena, uint64_t dbase,
                                                 const FastRows& t, int rows, uint32_t G) {
  const uint32_t* pre = kVal ? t.vpre : t.kpre;
  const uint32_t tid = threadIdx.x;
  const uint32_t grp = tid / G, sub = tid % G, ngrp = blockDim.x / G;
  for (uint32_t i = grp; i < uint32_t(rows); i += ngrp) {
    const uint32_t p0 = pre[i], p1 = pre[i + 1];
    if (p1 == p0) continue;
    const uint32_t cfirst = (p0 + 15) >> 4, clast = (p1 - 1) >> 4;
    const uint32_t si = bias + t.rec[i] + 6 + (kVal ? t.kpre[i + 1] - t.kpre[i] : 0u);
    for (uint32_t c = cfirst + sub; c <= clast; c += G) {
      const uint32_t cs = c << 4, ce = cs + 16;
      uint4 out = load16_lds_b128(s4, si + (cs - p0));
      if (ce > p1) {  // spills past row i: keep [0, p1-cs), gather the rest
        out = merge_bytes(make_uint4(0, 0, 0, 0), out, 0, int32_t(p1 - cs));
        for (uint32_t j = i + 1; j < uint32_t(rows) && pre[j] < ce; ++j) {
          const uint32_t q0 = pre[j], q1 = pre[j + 1];
          if (q1 == q0) continue;
          const uint32_t sj = bias + t.rec[j] + 6 + (kVal ? t.kpre[j + 1] - t.kpre[j] : 0u);
          const uint4 v = load16_lds_b128(s4, sj - (q0 - cs));
          out = merge_bytes(out, v, int32_t(q0 - cs), int32_t((q1 < ce ? q1 : ce) - cs));
        }
      }
      *reinterpret_cast<uint4*>(arena + dbase + cs) = out;
    }
  }
}

// SoA rows and both arena regions of a block staged in LDS whose row table
// (rec / kpre / vpre, <= kFastRows rows) is built.
__device__ __forceinline__ void emit_fast(const CopyParams& P, CopySmem& sm, uint32_t bias,
                                          int rows, uint64_t kbytes, uint64_t vbytes,
                                          uint64_t row0, uint64_t kb0, uint64_t vb0) {
  const uint32_t tid = threadIdx.x;
  FastRows& t = sm.f;
  for (int i = tid; i < rows; i += blockDim.x) {
    const uint64_t g = row0 + i;
    P.key_off[g] = kb0 + t.kpre[i];
    P.key_len[g] = uint16_t(t.kpre[i + 1] - t.kpre[i]);
    P.val_off[g] = vb0 + t.vpre[i];
    P.val_len[g] = t.vpre[i + 1] - t.vpre[i];
  }
  const uint32_t Gk = group_size(kbytes / rows), Gv = group_size(vbytes / rows);
  copy_region_fast<false>(sm.stage, bias, P.key_arena, kb0, t, rows, Gk);
  copy_region_fast<true>(sm.stage, bias, P.val_arena, vb0, t, rows, Gv);
}

__device__ __forceinline__ void materialise_fast(const CopyParams& P, CopySmem& sm,
                                                uint32_t bias, int rows, uint64_t kbytes,
                                                uint64_t vbytes, uint64_t row0, uint64_t kb0,
                                                uint64_t vb0) {
  const uint32_t tid = threadIdx.x;
  FastRows& t = sm.f;
  if (tid == 0) {
    // serial header chase in LDS: record i+1 starts at rec_i + 6 + klen_i + vlen_i
    // (lengths clamped to pass 1's totals: if the segment changed under the
    // decode, the walk still writes only inside this block's regions)
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(sm.stage);
    uint32_t p = 0, ka = 0, va = 0;
    for (int i = 0; i < rows; ++i) {
      uint32_t kl, vl;
      header_lds(sw, bias + p, kl, vl);
      kl = min(kl, uint32_t(kbytes) - ka);
      vl = min(vl, uint32_t(vbytes) - va);
      t.rec[i] = p;
      t.kpre[i] = ka;
      t.vpre[i] = va;
      ka += kl;
      va += vl;
      p = min(p + 6 + kl + vl, uint32_t(kStage));
    }
    t.rec[rows] = p;
    t.kpre[rows] = ka;
    t.vpre[rows] = va;
  }
  __syncthreads();
  emit_fast(P, sm, bias, rows, kbytes, vbytes, row0, kb0, vb0);
}

__global__ __launch_bounds__(kThreads) void okv_copy_kernel(CopyParams P) {
  __shared__ CopySmem sm;
  const uint32_t tid = threadIdx.x;
  const uint32_t nbig = *P.big_count;
  for (uint32_t k = blockIdx.x; k < nbig; k += gridDim.x) {
    const uint32_t b = P.big_list[k];
    const BlockCount c = P.cnt[b];
    const BlockBase B = block_base(P, b, c);
    if (B.st != OKV_BLK_OK) continue;  // status written by okv_gather_kernel
    const Desc d = P.descs[b];
    if (c.pend <= uint64_t(kStage)) {
      // stage [offset - shift, offset + pend) with aligned 16-byte loads
      const uint32_t shift = uint32_t(d.offset & 15);
      const uint32_t nch = uint32_t((shift + c.pend + 15) / 16);
      const uint4* g = reinterpret_cast<const uint4*>(P.seg + (d.offset - shift));
      for (uint32_t ci = tid; ci < nch; ci += kThreads) sm.stage[1 + ci] = load_nt16(g + ci);
      __syncthreads();
      if (c.rows <= uint64_t(kFastRows)) {
        materialise_fast(P, sm, 16u + shift, int(c.rows), c.kbytes, c.vbytes, B.row0, B.kb0,
                            B.vb0);
      } else {
        const Staged src{sm.stage, 16u + shift};
        materialise(src, P, sm, c.rows, c.kbytes, c.vbytes, B.row0, B.kb0, B.vb0, c.pend);
      }
    } else {
      GlobalSrc src{P.seg, P.seg_bytes, d.offset};
      materialise(src, P, sm, c.rows, c.kbytes, c.vbytes, B.row0, B.kb0, B.vb0, c.pend);
    }
    __syncthreads();  // LDS is reused by the next big block
  }
}

// ---------------------------------------------------------------------------
// Point reads: a host-mode call of a few small uncompressed blocks (GetRow's
// one block, GetRange's few; segment_reader.go:362-404, :410-475).  One
// workgroup decodes the batch block after block, reading the staged bytes
// straight from the context's pinned slab and writing every output into it,
// so the call is one launch and one synchronisation (no H2D / D2H copies,
// no plan, no totals read-back).  Per block: the block's
// bytes into LDS (one trip over PCIe), the header walk in LDS by wave 0
// (walk_staged_to: Go's checks in its order, :338-352), recording the row table
// as it goes, then the SoA rows and both arena regions from LDS (emit_fast;
// blocks of more than kFastRows rows re-walk in batches, materialise).  The
// host admits only batches whose OK blocks stage (BlockSize <= kStage).
// The kernel is its phases: point_block, then point_find or point_rows.
// ---------------------------------------------------------------------------
#ifdef OKV_ABLATE
// (ablation build: wall-clock stamps of the point kernel's phases for the
// last block of the last call -- start, staged, walked, prefixes, emitted;
// okv_debug_point_times, tools/point_phases.py)
__device__ uint64_t g_point_t[8];
#define OKV_POINT_STAMP(i) \
  if (tid == 0) g_point_t[i] = wall_clock64()
#else
#define OKV_POINT_STAMP(i)
#endif
// okv_point_get's search (GetRow :395-403): the key (<= kFindKey bytes, host
// memory, 4-byte aligned) and the answer: found = 1 (the row's key and value
// at key_arena / val_arena, lengths at key_len[0] / val_len[0]), 0, or -1
// (more rows than the row table: the caller decodes the block in full).
struct PointFind {
  const uint8_t* key;
  uint32_t klen;
  int32_t* found;
  uint32_t* done;  // non-null: the call's completion word in the pinned slab (point_wait)
  uint32_t seq;    // ... the value the kernel writes there last
};
// The kernel's last act: every wave's slab writes pushed to system scope,
// then one store of the call's sequence number, for which the host spins
// (point_wait) instead of waiting in hipStreamSynchronize.
__device__ __forceinline__ void point_done(const PointFind& F) {
  if (!F.done) return;
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(F.done, F.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
constexpr uint32_t kFindKey = 8192;  // (held in the row table's prefix arrays)

// What every thread knows of a point call's block once it is staged and walked, and the
// words wave 0 hands it over in.
struct PointBlock {
  Staged src;
  int32_t st;
  uint64_t rows, kb, vb, pend;
};
struct PointWalk {
  uint64_t rows, kb, vb, pend;
  int32_t st;
};

// Block b into LDS (every 16-byte piece in flight at once -- a load/store loop paid one
// PCIe round trip per iteration, ~16 for a 64 KiB block), then its header walk by wave 0
// (lane 0 alone, one dependent header decode per record: 120 ns a record, 80 us of a
// 64 KiB block's GetRow), the positions of rows < kFastRows into the row table, and the
// block's outputs at the running prefix `at`.
__device__ __forceinline__ PointBlock point_block(const CopyParams& P, uint32_t b,
                                                  const Prefix& at, CopySmem& sm, PointWalk& w) {
  const uint32_t tid = threadIdx.x;
  OKV_POINT_STAMP(0);
  const Desc d = P.descs[b];
  uint64_t len;
  const int32_t st0 = entry_status(d, P.seg_bytes, P.comp, nullptr, b, len);
  const uint32_t L = st0 == OKV_BLK_OK ? uint32_t(len) : 0u;  // <= kStage (point_eligible)
  const Staged src{sm.stage, stage_block_wg<kThreads>(sm.stage, P.seg, d.offset, L)};
  __syncthreads();
  OKV_POINT_STAMP(1);
  if (tid < 64) {
    int32_t st = st0;
    uint64_t rows = 0, kb = 0, vb = 0, pend = 0;
    if (st == OKV_BLK_OK)
      walk_staged_to(src, L, d.original_size, RecSink{sm.f.rec, kFastRows}, tid, st, rows, kb, vb,
                     pend);
    if (tid == 0) {
      w = PointWalk{rows, kb, vb, pend, st};
      P.row_start[b] = at.rows;
      P.key_base[b] = at.kb;
      P.val_base[b] = at.vb;
      P.blk_status[b] = st;
    }
  }
  __syncthreads();
  OKV_POINT_STAMP(2);
  return PointBlock{src, w.st, w.rows, w.kb, w.vb, w.pend};
}

// okv_point_get's answer from its walked block: the first row whose key equals the
// probe (in LDS, over the prefix arrays: unused by the search) -- one lane per row
// compares, the lowest index wins -- and only that row's bytes go back.
__device__ __forceinline__ void point_find(const CopyParams& P, Totals* tot, const PointFind& F,
                                           const CopySmem& sm, const PointBlock& k) {
  __shared__ uint32_t s_hit;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_hit = ~0u;
  __syncthreads();
  const bool ok = k.st == OKV_BLK_OK, listed = k.rows <= uint64_t(kFastRows);
  if (ok && listed) {
    const uint32_t* tk = sm.k.key;
    for (uint32_t i = tid; i < uint32_t(k.rows); i += kThreads)
      if (key_equal(k.src, sm.f.rec[i], F.klen, [tk](uint32_t j) { return tk[j >> 2]; }))
        atomicMin(&s_hit, i);
  }
  __syncthreads();
  OKV_POINT_STAMP(3);
  const uint32_t hit = s_hit;
  uint32_t kl = 0, vl = 0;
  if (hit != ~0u) {
    const uint32_t r0 = sm.f.rec[hit];
    k.src.header(r0, kl, vl);
    uint4* ka = reinterpret_cast<uint4*>(P.key_arena);
    uint4* va = reinterpret_cast<uint4*>(P.val_arena);
    for (uint32_t c = tid; c < (kl + 15) / 16; c += kThreads) ka[c] = k.src.load16(r0 + 6 + 16 * c);
    for (uint32_t c = tid; c < (vl + 15) / 16; c += kThreads)
      va[c] = k.src.load16(r0 + 6 + kl + 16 * c);
  }
  if (tid == 0) {
    *F.found = !ok ? 0 : !listed ? -1 : hit != ~0u ? 1 : 0;
    P.key_len[0] = uint16_t(kl);
    P.val_len[0] = vl;
    *tot = Totals{hit != ~0u ? 1u : 0u, kl, vl, uint64_t(!ok)};
  }
  OKV_POINT_STAMP(4);
}

// A walked block's rows out.  Up to kFastRows rows: the recorded rows' key and value
// lengths (4 rows a lane), their exclusive prefixes by two workgroup scans (DPP in the
// wave, the waves' sums through s_wsum), then the SoA rows and both arena regions from
// LDS (emit_fast).  More rows than the table holds: the batched row tables
// (materialise), with the walk's byte totals.
__device__ __forceinline__ void point_rows(const CopyParams& P, CopySmem& sm,
                                           uint32_t (*s_wsum)[kThreads / 64],
                                           const PointBlock& k, const Prefix& at) {
  const uint32_t tid = threadIdx.x;
  if (k.rows > uint64_t(kFastRows)) {
    materialise(k.src, P, sm, k.rows, k.kb, k.vb, at.rows, at.kb, at.vb, k.pend);
    return;
  }
  constexpr int kPer = kFastRows / kThreads;
  const uint32_t rows = uint32_t(k.rows);
  uint32_t kls[kPer], vls[kPer], ks = 0, vs = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint32_t i = tid * kPer + j;
    kls[j] = vls[j] = 0;
    if (i < rows) k.src.header(sm.f.rec[i], kls[j], vls[j]);
    ks += kls[j];
    vs += vls[j];
  }
  const uint32_t ki = wave_scan_dpp(ks), vi = wave_scan_dpp(vs), wave = tid >> 6;
  if ((tid & 63) == 63) {
    s_wsum[0][wave] = ki;
    s_wsum[1][wave] = vi;
  }
  __syncthreads();
  uint32_t kx = ki - ks, vx = vi - vs;
#pragma unroll
  for (uint32_t w = 0; w < kThreads / 64; ++w) {
    kx += w < wave ? s_wsum[0][w] : 0u;
    vx += w < wave ? s_wsum[1][w] : 0u;
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint32_t i = tid * kPer + j;
    if (i < rows) {
      sm.f.kpre[i] = kx;
      sm.f.vpre[i] = vx;
    }
    kx += kls[j];
    vx += vls[j];
  }
  // (32-bit totals, <= 64 KiB: emit_fast's bytes-per-row divisions stay 32-bit)
  const uint32_t kb = uint32_t(k.kb), vb = uint32_t(k.vb);
  if (tid == 0) {
    sm.f.rec[rows] = uint32_t(k.pend);
    sm.f.kpre[rows] = kb;
    sm.f.vpre[rows] = vb;
  }
  __syncthreads();
  OKV_POINT_STAMP(3);
  emit_fast(P, sm, k.src.bias, int(rows), kb, vb, at.rows, at.kb, at.vb);
}

template <bool kFind>
__global__ __launch_bounds__(kThreads) void okv_point_kernel(CopyParams P, Totals* tot,
                                                             PointFind F) {
  __shared__ CopySmem sm;
  __shared__ PointWalk s_w;
  Prefix at{0, 0, 0, 0};  // rows, padded key and value bytes, failed blocks so far (uniform)
  if constexpr (kFind) {  // one block; the key into LDS before the block's barriers
    static_assert(sizeof(sm.k.key) >= kFindKey, "the key fits its LDS array");
    const uint32_t* k4 = reinterpret_cast<const uint32_t*>(F.key);
    for (uint32_t i = threadIdx.x; i < (F.klen + 3) / 4; i += kThreads) sm.k.key[i] = k4[i];
    point_find(P, tot, F, sm, point_block(P, 0, at, sm, s_w));
  } else {
    __shared__ uint32_t s_wsum[2][kThreads / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t b = 0; b < P.nblk; ++b) {
      const PointBlock k = point_block(P, b, at, sm, s_w);
      if (k.st == OKV_BLK_OK && k.rows) point_rows(P, sm, s_wsum, k, at);
      at.rows += k.rows;
      at.kb += round16(k.kb);
      at.vb += round16(k.vb);
      at.bad += k.st != OKV_BLK_OK;
      __syncthreads();  // the stage and the row table are reused by the next block
      OKV_POINT_STAMP(4);
    }
    if (tid == 0) {
      P.row_start[P.nblk] = at.rows;
      *tot = Totals{at.rows, at.kb, at.vb, at.bad};
    }
  }
  point_done(F);
}

// ---------------------------------------------------------------------------
// OKV_F_INDEX_ONLY for big blocks: one lane per block re-walks the headers.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void okv_index_kernel(CopyParams P) {
  const uint32_t nbig = *P.big_count;
  for (uint32_t k = blockIdx.x * kThreads + threadIdx.x; k < nbig; k += gridDim.x * kThreads) {
    const uint32_t b = P.big_list[k];
    const BlockCount c = P.cnt[b];
    const BlockBase B = block_base(P, b, c);
    if (B.st != OKV_BLK_OK) continue;
    const uint64_t off = P.descs[b].offset;
    uint64_t p = 0;
    for (uint64_t r = 0; r < c.rows; ++r) {
      uint32_t kl, vl;
      header_global(P.seg, off + p, kl, vl);
      const uint64_t g = B.row0 + r;
      P.key_off[g] = off + p + 6;
      P.key_len[g] = uint16_t(kl);
      P.val_off[g] = off + p + 6 + kl;
      P.val_len[g] = vl;
      // (clamped to pass 1's walk end: reads stay in the block if the segment
      // changed under the decode)
      p = min<uint64_t>(p + 6 + uint64_t(kl) + uint64_t(vl), c.pend - 6);
    }
  }
}

// ---------------------------------------------------------------------------
// XXH64 of each block's BlockSize bytes (BlockStat.Hash, segment_writer.go:185).
// XXH64 has four independent accumulators, so four lanes share one block
// (lane q owns stripe word q); the merge and tail run on lane q == 0.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void okv_hash_kernel(const uint8_t* __restrict__ seg,
                                                            uint64_t seg_bytes,
                                                            const Desc* __restrict__ descs,
                                                            uint32_t nblk,
                                                            uint64_t* __restrict__ out) {
  const uint32_t gid = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t b = gid >> 2, q = gid & 3;
  const bool live = b < nblk;
  Desc d = {0, 0, 0, 0};
  if (live) d = descs[b];
  const bool ok = live && d.offset < seg_bytes && seg_bytes - d.offset >= d.block_size;
  const uint8_t* p = seg + (ok ? d.offset : 0);
  const uint64_t len = ok ? d.block_size : 0;
  const uint64_t nstripe = len / 32;
  const uint64_t seed = 0;
  uint64_t acc = (q == 0) ? seed + XP1 + XP2 : (q == 1) ? seed + XP2 : (q == 2) ? seed : seed - XP1;
  const bool aligned = ((reinterpret_cast<uintptr_t>(p)) & 7) == 0;
  for (uint64_t s = 0; s < nstripe; ++s) {
    const uint8_t* w = p + s * 32 + q * 8;
    const uint64_t x = aligned ? *reinterpret_cast<const uint64_t*>(w) : ld64u(w);
    acc = xround(acc, x);
  }
  // gather the four accumulators onto lane q == 0 of the quad
  const int lane = threadIdx.x & 63;
  const uint64_t a1 = __shfl(acc, (lane & ~3) + 1, 64);
  const uint64_t a2 = __shfl(acc, (lane & ~3) + 2, 64);
  const uint64_t a3 = __shfl(acc, (lane & ~3) + 3, 64);
  if (!live || q != 0) return;
  if (!ok) {
    out[b] = 0;
    return;
  }
  uint64_t h;
  if (len >= 32) {
    const uint64_t v1 = acc, v2 = a1, v3 = a2, v4 = a3;
    h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
    h = (h ^ xround(0, v1)) * XP1 + XP4;
    h = (h ^ xround(0, v2)) * XP1 + XP4;
    h = (h ^ xround(0, v3)) * XP1 + XP4;
    h = (h ^ xround(0, v4)) * XP1 + XP4;
  } else {
    h = seed + XP5;
  }
  h += len;
  const uint8_t* t = p + nstripe * 32;
  const uint8_t* end = p + len;
  while (t + 8 <= end) {
    h ^= xround(0, ld64u(t));
    h = rotl64(h, 27) * XP1 + XP4;
    t += 8;
  }
  if (t + 4 <= end) {
    const uint32_t v = uint32_t(t[0]) | (uint32_t(t[1]) << 8) | (uint32_t(t[2]) << 16) |
                       (uint32_t(t[3]) << 24);
    h ^= uint64_t(v) * XP1;
    h = rotl64(h, 23) * XP2 + XP3;
    t += 4;
  }
  while (t < end) {
    h ^= uint64_t(*t) * XP5;
    h = rotl64(h, 11) * XP1;
    ++t;
  }
  h ^= h >> 33;
  h *= XP2;
  h ^= h >> 29;
  h *= XP3;
  h ^= h >> 32;
  out[b] = h;
}

void launch_hash(hipStream_t stream, const uint8_t* seg, uint64_t seg_bytes, const Desc* descs,
                 uint32_t nblk, uint64_t* out) {
  if (!nblk) return;
  const uint64_t threads = uint64_t(nblk) * 4;
  hipLaunchKernelGGL(okv_hash_kernel, dim3(uint32_t((threads + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, stream, seg, seg_bytes, descs, nblk, out);
}

#ifdef OKV_ABLATE  // the look-back stream kernel (ablation build only)
#include "okv_decode_ablate_lb.inc"
#endif
}  // namespace okv

// ===========================================================================
// C-ABI (include/okv_sst.h)
// ===========================================================================
using namespace okv;

namespace {

int ensure_blocks(okv_ctx* ctx, uint32_t nblk) {
  const size_t n = std::max<size_t>(nblk, 1);
  const size_t ntiles = (n + kTile - 1) / kTile;
  bool fresh = false;
  int rc;
  if ((rc = reserve(ctx, ctx->d_ctr, 16, &fresh))) return rc;
  if (fresh) {
    OKV_HIP(hipMemsetAsync(ctx->d_ctr.data(), 0, ctx->d_ctr.bytes(), ctx->stream));
    ctx->big_slot = 0;
  }
  if ((rc = reserve(ctx, ctx->d_rec, n * kRCap)) || (rc = reserve(ctx, ctx->d_big, n + 1)) ||
      (rc = reserve(ctx, ctx->d_cnt, n)) || (rc = reserve(ctx, ctx->d_lp, n)) ||
      (rc = reserve(ctx, ctx->d_tile_tot, ntiles + 1)))
    return rc;
  return reserve(ctx, ctx->d_tile_pre, ntiles + 1);
}

// Counters kept across calls (zeroed once): the count kernel's arrival
// counter (reset by its last workgroup) and two big-block counter slots.  A
// launch uses slot big_slot and zeroes the other one, which the next launch
// uses: its previous readers (the kernels of the decode before) have completed
// by then, so no memset launch is needed per decode.
constexpr uint32_t kCtrArrive = 0, kCtrBig = 1;
uint32_t* big_counter(okv_ctx* ctx, uint32_t other = 0) {
  return ctx->d_ctr.data() + kCtrBig + (ctx->big_slot ^ other);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Event slot k (0..kProfEv-1) of the current timed call, or nullptr when not
// profiling: 0 start, 1 zstd stage done, 2 pass 1 done, 3 pass 2 done, 4 end.
constexpr int kProfEv = 5;
hipEvent_t prof_event(okv_ctx* ctx, int k) {
  if (!ctx->prof) return nullptr;
  const size_t need = ctx->ev_used + kProfEv;
  while (ctx->ev.size() < need) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    ctx->ev.push_back(e);
  }
  return ctx->ev[ctx->ev_used + k];
}

void prof_mark(okv_ctx* ctx, int k) {
  hipEvent_t e = prof_event(ctx, k);
  if (e) (void)hipEventRecord(e, ctx->stream);
  if (e && k == kProfEv - 1) ctx->ev_used += kProfEv;
}

// Working inputs of passes 1-3: the segment itself, or for zstd blocks the
// decompressed bytes (okv_zstd.hip) with per-block statuses from that stage.
struct Work {
  const uint8_t* seg;
  uint64_t seg_bytes;
  const Desc* descs;
  int comp;
  const int32_t* pre;
  uint32_t retried;  // zstd blocks decoded again into a larger region (0: no zstd stage ran)
};

int prepare(okv_ctx* ctx, const uint8_t* d_seg, uint64_t seg_bytes, const Desc* d_desc,
            uint32_t nblk, int comp, bool index_only, Work* w) {
  *w = Work{d_seg, seg_bytes, d_desc, comp, nullptr, 0};
  if (comp != OKV_COMP_ZSTD || index_only || nblk == 0) return OKV_OK;
  ZstdOut z;
  const int rc = zstd_stage(ctx, d_seg, seg_bytes, d_desc, nblk, &z);
  if (rc) return rc;
  *w = Work{z.bytes, z.n_bytes, z.descs, OKV_COMP_NONE, z.status, z.retried};
  return OKV_OK;
}

// Pass-3 workgroup width from the call's average block span (seg_bytes /
// nblk: it assumes the blocks tile the segment, which holds for whole-segment
// decodes; a caller decoding a few blocks of a large segment gets the
// 256-thread form, which is correct for any block size).
uint32_t gather_threads(const Work& w, uint32_t nblk) {
  return nblk && w.seg_bytes / nblk <= 16384 ? 64u : 256u;
}

// Tile-pass geometry (okv_tile_kernel): tiles per block from the call's
// average block span, rounded down to 4 KiB (a segment's meta block and
// trailer add far less than that per block); blocks whose walk ends past
// tpb tiles are big blocks (okv_copy_kernel).  Index-only decodes write only
// the row index: one workgroup per block, no span limit.
struct TileGeo {
  uint32_t tpb;
  uint64_t span_cap;
};
constexpr uint32_t kTileBytes = 16384;  // the product tile pass's source tile

// The ablation build's hooks into the functions below (okv_decode_ablate_host.inc).
[[maybe_unused]] int ablate_count_prefetch(int prefetch, uint32_t nblk);
[[maybe_unused]] void ablate_launch_tile(okv_ctx* ctx, const CopyParams& P, const TileGeo& g);

// Launch passes 1 and 2 on device inputs (the caller has run ensure_blocks).
// rt_kl: record key lengths for the tile pass (null: positions only);
// span_cap: blocks whose walk ends past it go to the big-block list.
int launch_plan(okv_ctx* ctx, const Work& w, uint32_t nblk, uint64_t* d_row_start,
                bool timed = false, uint16_t* rt_kl = nullptr, uint64_t span_cap = ~0ull,
                unsigned long long* span_max = nullptr) {
  // one launch: the count walk, and the tile-total scan by its last workgroup
  // (an empty batch still runs one workgroup: it writes the zero totals)
  const uint32_t ntiles = std::max<uint32_t>(1, (nblk + kTile - 1) / kTile);
  // prefetch block lines before the chase when the segment fits in the caches
  // and blocks are small (dense headers); 64 KiB blocks touch ~5 % of their lines
  int prefetch = nblk && w.seg_bytes <= (64ull << 20) && w.seg_bytes / nblk <= 16384;
#ifdef OKV_ABLATE
  prefetch = ablate_count_prefetch(prefetch, nblk);  // OKV_COUNT_PREFETCH A/B
#endif
  hipLaunchKernelGGL(okv_count_kernel, dim3(ntiles), dim3(kThreads), 0, ctx->stream, w.seg,
                     w.seg_bytes, w.descs, nblk, w.comp, ctx->d_cnt.data(), ctx->d_lp.data(),
                     ctx->d_tile_tot.data(), ctx->d_rec.data(), rt_kl, ctx->d_big.data(),
                     big_counter(ctx), w.pre, prefetch, span_cap, ctx->d_tile_pre.data(),
                     ctx->d_tot.data(), d_row_start, ctx->d_ctr.data() + kCtrArrive,
                     big_counter(ctx, 1), nullptr, 0u, span_max);
  OKV_HIP(hipGetLastError());
  ctx->big_slot ^= 1u;  // the launch zeroes the other slot: the next launch's counter
  if (timed) prof_mark(ctx, 2);  // (the caller marks 3: after the big-block kernel)
  return OKV_OK;
}

// ... or from the longest walk the last okv_decode_plan of the same batch
// measured (with bimodal block sizes most bytes would be big blocks' otherwise).
TileGeo tile_geo(const okv_ctx* ctx, const Work& w, uint32_t nblk, bool index_only,
                 uint64_t tile = kTileBytes) {
  if (index_only || !nblk) return {1, ~0ull};
  uint64_t span = (w.seg_bytes / nblk) & ~uint64_t(4095);
  if (span < 4096) span = 4096;
  const SpanHint& h = ctx->span_hint;
  if (h.nblk == nblk && h.seg == w.seg && h.descs == w.descs && h.seg_bytes == w.seg_bytes)
    span = std::max<uint64_t>(span, (h.span + 4095) & ~uint64_t(4095));
  // (the hint is consumed by the decode that uses it -- decode_device clears
  // it -- so a later batch staged into the same buffers is not sized by it)
  uint64_t tpb = std::min<uint64_t>(64, (span + tile - 1) / tile);
  while (tpb > 1 && uint64_t(nblk) * tpb >= (uint64_t(1) << 31)) tpb >>= 1;
  return {uint32_t(tpb), tpb * tile};
}

// The tile pass over P's blocks: kTileBytes source tiles, 256 threads,
// consecutive tiles on one XCD (the grid padded to a multiple of 8).
void launch_tile(okv_ctx* ctx, const CopyParams& P, const TileGeo& g) {
#ifdef OKV_ABLATE
  ablate_launch_tile(ctx, P, g);  // the OKV_TILE form (default: the product form)
#else
  const uint32_t ntile = P.nblk * g.tpb;
  hipLaunchKernelGGL((okv_tile_kernel<kTileBytes, 256, true>), dim3((ntile + 7u) & ~7u),
                     dim3(256), 0, ctx->stream, P, g.tpb, ntile);
#endif
}

// The record key lengths pass 1 leaves for the tile pass (count kernel rt_kl).
int ensure_hdr(okv_ctx* ctx, uint32_t nblk, uint16_t** rt_kl) {
  const int rc = reserve(ctx, ctx->d_hdr, size_t(nblk) * kRCap);
  *rt_kl = ctx->d_hdr.data();
  return rc;
}

// Look-back scratch of a single-pass decode: n flags, zeroed once per
// allocation (the epoch tag makes every call's flags fresh), and n aggregate
// and inclusive prefixes.
template <class Flag>
int ensure_lookback(okv_ctx* ctx, size_t n, DevBuf<Flag>& flag, DevBuf<Prefix>& agg,
                    DevBuf<Prefix>& incl) {
  n = std::max<size_t>(n, 1);
  bool fresh = false;
  int rc;
  if ((rc = reserve(ctx, flag, n, &fresh))) return rc;
  if (fresh) OKV_HIP(hipMemsetAsync(flag.data(), 0, flag.bytes(), ctx->stream));
  if ((rc = reserve(ctx, agg, n))) return rc;
  return reserve(ctx, incl, n);
}

// Scratch of okv_decode_fused_kernel: one 8-byte look-back word per block (the
// ablation stream kernel uses the first 4 bytes per block as its flags).
int ensure_fused(okv_ctx* ctx, uint32_t nblk) {
  bool fresh = false;
  int rc;
  if ((rc = ensure_lookback(ctx, nblk, ctx->f_flag, ctx->f_agg, ctx->f_incl)) ||
      (rc = reserve(ctx, ctx->f_ctr, 2, &fresh)))  // blocks, arrivals
    return rc;
  if (fresh) {
    OKV_HIP(hipMemsetAsync(ctx->f_ctr.data(), 0, ctx->f_ctr.bytes(), ctx->stream));
    ctx->f_base = 0;
  }
  return OKV_OK;
}

// Pass-3 parameters of a device-pointer decode.  big_count is this decode's
// big-block counter slot: call before the launch that flips big_slot.
CopyParams copy_params(okv_ctx* ctx, const Work& w, uint32_t nblk, bool index_only,
                       uint16_t* rt_kl, uint64_t span_cap, const okv_decode_out& o) {
  CopyParams P = {};  // (vsrc, vtile, bchunk: null -- the ablation sweep's)
  P.seg = w.seg;
  P.seg_bytes = w.seg_bytes;
  P.descs = w.descs;
  P.nblk = nblk;
  P.comp = w.comp;
  P.index_only = index_only ? 1 : 0;
  P.rt_pos = ctx->d_rec.data();
  P.rt_kl = rt_kl;
  P.span_cap = span_cap;
  P.big_list = ctx->d_big.data();
  P.big_count = big_counter(ctx);
  P.cnt = ctx->d_cnt.data();
  P.lp = ctx->d_lp.data();
  P.tile_pre = ctx->d_tile_pre.data();
  P.row_start = o.row_start;
  P.key_base = o.key_base;
  P.val_base = o.val_base;
  P.blk_status = o.blk_status;
  P.key_off = o.key_off;
  P.key_len = o.key_len;
  P.val_off = o.val_off;
  P.val_len = o.val_len;
  P.key_arena = o.key_arena;
  P.val_arena = o.val_arena;
  P.row_cap = o.row_cap;
  P.key_cap = index_only ? 0 : o.key_cap;
  P.val_cap = index_only ? 0 : o.val_cap;
  P.tot = ctx->d_tot.data();
  return P;
}

// Parameters of the single-pass kernels; starts the call's epoch.
FusedParams fused_params(okv_ctx* ctx, const Work& w) {
  ctx->f_epoch = (ctx->f_epoch + 1) & 0x3fffffffu;
  uint32_t* flag = reinterpret_cast<uint32_t*>(ctx->f_flag.data());
  unsigned long long* ctr = ctx->f_ctr.data();
  return FusedParams{w.pre, ctx->d_cnt.data(), ctx->d_lp.data(), ctx->d_tile_pre.data(), flag,
                     ctx->f_agg.data(), ctx->f_incl.data(), ctr, ctr + 1, ctx->f_base,
                     ctx->f_epoch, ctx->d_tot.data(), big_counter(ctx, 1)};
}

// The big-block kernel: the blocks of the big-block list (more than kRCap
// rows, or a walk past the tile span), a no-op grid when the list is empty.
void launch_big(okv_ctx* ctx, const CopyParams& P) {
  const uint32_t grid = std::min<uint32_t>(P.nblk, 512);
  if (P.index_only)
    hipLaunchKernelGGL(okv_index_kernel, dim3((grid + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       ctx->stream, P);
  else
    hipLaunchKernelGGL(okv_copy_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, P);
}

// okv_decode_chain: pass 3 after the chained context's last pass 3.  (A
// shared pass-3 stream for chained contexts instead of this event wait
// measured slower: C5 0.407 vs 0.396 ms, C3 1.465 vs 1.449 ms per step with
// decodes in flight, profiles/r6/session/pass3_queue_ab.log.)
int chain_wait(okv_ctx* ctx) {
  if (ctx->chain && ctx->chain->p3_rec)
    OKV_HIP(hipStreamWaitEvent(ctx->stream, ctx->chain->p3_done, 0));
  return OKV_OK;
}

int read_totals(okv_ctx* ctx, Totals* out) {
  OKV_HIP(hipMemcpyAsync(ctx->h_tot.data(), ctx->d_tot.data(), sizeof(Totals),
                         hipMemcpyDeviceToHost, ctx->stream));
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  *out = *ctx->h_tot;
  return OKV_OK;
}

// A decode's totals into the caller's okv_decode_out; false when they exceed
// its capacities (index-only decodes have no arenas).
bool totals_fit(const Totals& T, bool index_only, okv_decode_out* o) {
  o->n_rows = T.rows;
  o->key_bytes = index_only ? 0 : T.kb;
  o->val_bytes = index_only ? 0 : T.vb;
  o->n_bad_blocks = T.bad;
  return T.rows <= o->row_cap && (index_only || (T.kb <= o->key_cap && T.vb <= o->val_cap));
}

// After the pass-3 launches: the event chained contexts wait for, the last
// profile mark and, unless the call is OKV_F_ASYNC, the totals.
int finish_decode(okv_ctx* ctx, okv_decode_out* o, uint32_t flags) {
  if (ctx->p3_done) {
    OKV_HIP(hipEventRecord(ctx->p3_done, ctx->stream));
    ctx->p3_rec = true;
  }
  prof_mark(ctx, 4);
  if (flags & OKV_F_ASYNC) return OKV_OK;
  Totals T;
  const int rc = read_totals(ctx, &T);
  if (rc) return rc;
  if (!totals_fit(T, flags & OKV_F_INDEX_ONLY, o))
    return set_err(ctx, OKV_E_CAPACITY, "output capacity too small (totals set)");
  return OKV_OK;
}

// okv_last_path of a decode: the compression stage's bits and the kernels'.
// w: the decode's prepared inputs (the zstd stage's retry count).
uint32_t path_bits(const Work& w, int comp, bool index_only, uint32_t kernels) {
  return (comp ? OKV_PATH_ZSTD : 0u) |
         (comp == OKV_COMP_ZSTD && !index_only && w.retried ? OKV_PATH_ZSTD_REGROW : 0u) |
         kernels;
}

#ifdef OKV_ABLATE  // the measured alternative forms and their knobs (ablation build only)
#include "okv_decode_ablate_host.inc"
#endif

// The product's decode routes; each value is the route's okv_last_path bits.
// Every route but kEmpty ends with the big-block kernel (launch_big).
enum class Route : uint32_t {
  kEmpty = 0,                              // no blocks: the count launch writes the zero totals
  kFused = OKV_PATH_FUSED,                 // passes 1-3 in one launch (okv_decode_fused_kernel)
  kSmall = OKV_PATH_BIG | OKV_PATH_SMALL,  // count, then okv_gather_small_kernel
  kTile = OKV_PATH_BIG | OKV_PATH_TILE,    // count, then okv_tile_kernel
};
// Blocks averaging more than 16 KiB take the tile pass; small blocks the fused
// kernel while the batch fits its resident grid (fused_max; a context opened
// with OKV_OPEN_NO_FUSED never), else the count launch and the small gather.
Route select_route(const okv_ctx* ctx, const Work& w, uint32_t nblk) {
  if (!nblk) return Route::kEmpty;
  if (gather_threads(w, nblk) == 256) return Route::kTile;
  return ctx->fused && nblk <= ctx->fused_max ? Route::kFused : Route::kSmall;
}

int decode_device(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes, const Desc* descs,
                  uint32_t nblk, int comp, okv_decode_out* o, uint32_t flags) {
  const bool index_only = flags & OKV_F_INDEX_ONLY;
  if (!o->row_start || !o->blk_status) return set_err(ctx, OKV_E_ARG, "row_start/blk_status");
  if (!aligned16(seg)) return set_err(ctx, OKV_E_ARG, "device seg must be 16-byte aligned");
  if (!index_only && (!aligned16(o->key_arena) || !aligned16(o->val_arena)))
    return set_err(ctx, OKV_E_ARG, "device arenas must be 16-byte aligned");
  prof_mark(ctx, 0);
  Work w;
  int rc = prepare(ctx, seg, seg_bytes, descs, nblk, comp, index_only, &w);
  if (rc) return rc;
  prof_mark(ctx, 1);
#ifdef OKV_ABLATE
  if (ctx->ab.active) return ablate_decode(ctx, w, nblk, comp, o, flags);  // a knob selects an arm
#endif
  const Route route = select_route(ctx, w, nblk);
  const bool tile = route == Route::kTile;
  const TileGeo geo = tile ? tile_geo(ctx, w, nblk, index_only) : TileGeo{1, ~0ull};
  ctx->span_hint = SpanHint{};  // a plan's hint sizes the one decode that follows it
  // scratch
  uint16_t* rt_kl = nullptr;
  if ((rc = ensure_blocks(ctx, nblk))) return rc;
  if (tile && (rc = ensure_hdr(ctx, nblk, &rt_kl))) return rc;
  if (route == Route::kFused && (rc = ensure_fused(ctx, nblk))) return rc;
  const CopyParams P = copy_params(ctx, w, nblk, index_only, rt_kl, geo.span_cap, *o);
  ctx->last_path = path_bits(w, comp, index_only, uint32_t(route));
  // passes 1-2.  When they are the count launch, the big-block kernel runs
  // right behind it: before the chained context's pass-3 wait, so with decodes
  // in flight it runs under the other decode's pass 3 (the list is empty on
  // C1-C5: an empty launch cost 4.6 us + a kernel boundary in front of each
  // pass 3), and before the pass-3 mark, so the pass-3 interval times the tile
  // / gather kernel alone.  The fused kernel does passes 1-2 itself.
  if (route == Route::kFused) {
    prof_mark(ctx, 2);
  } else {
    if ((rc = launch_plan(ctx, w, nblk, o->row_start, true, rt_kl, geo.span_cap))) return rc;
    if (route != Route::kEmpty) {
      launch_big(ctx, P);
      OKV_HIP(hipGetLastError());
    }
  }
  prof_mark(ctx, 3);
  if ((rc = chain_wait(ctx))) return rc;
  // pass 3
  switch (route) {
    case Route::kEmpty:
      break;
    case Route::kFused: {
      hipLaunchKernelGGL(okv_decode_fused_kernel, dim3(nblk), dim3(64), 0, ctx->stream, P,
                         fused_params(ctx, w));
      const hipError_t le = hipGetLastError();
      if (le != hipSuccess) return set_err(ctx, OKV_E_HIP, "okv_decode_fused_kernel launch", le);
      ctx->big_slot ^= 1u;  // the kernel zeroed the other slot (see big_counter)
      launch_big(ctx, P);
      break;
    }
    case Route::kSmall:
      hipLaunchKernelGGL(okv_gather_small_kernel, dim3(nblk), dim3(64), 0, ctx->stream, P);
      break;
    case Route::kTile:
      launch_tile(ctx, P, geo);
      break;
  }
  if (route != Route::kEmpty) OKV_HIP(hipGetLastError());
  return finish_decode(ctx, o, flags);
}

// Upper bounds of a host-mode decode's outputs from the host descriptors
// (uncompressed blocks: a block's records lie in its BlockSize bytes inside
// the segment, each >= 6 bytes; every block region pads to 16 bytes), or
// false when they do not exist (zstd: decompressed sizes) or exceed `limit`.
bool output_bounds(const uint8_t* /*seg*/, uint64_t seg_bytes, const okv_block_desc* descs,
                   uint32_t nblk, int comp, uint64_t limit, uint64_t* rows, uint64_t* bytes) {
  if (comp == OKV_COMP_ZSTD) return false;
  uint64_t r = 0, by = 0;
  for (uint32_t b = 0; b < nblk; ++b) {
    const okv_block_desc& d = descs[b];
    uint64_t span = 0;
    if (comp != OKV_COMP_LZ4 && int64_t(d.offset) >= 0 && d.offset < seg_bytes)
      span = std::min<uint64_t>(d.block_size, seg_bytes - d.offset);
    r += span / 6;
    by += span + 16;
    if (by > limit) return false;
  }
  *rows = r;
  *bytes = by;
  return true;
}

// ---- point reads (okv_point_kernel) -----------------------------------------
// A host-mode call goes through the point path when it is a few uncompressed
// (or LZ4-flagged) blocks whose readable blocks each fit the LDS stage: the
// shim's GetRow reads one block, GetRange the few its btree walks select.
constexpr uint32_t kPointMaxBlocks = 16;
constexpr uint64_t kPointMaxBytes = uint64_t(512) << 10;  // (1 MiB of 64 KiB blocks: 409 vs 309 us
// for the staged device path; 256 KiB: 111 vs 233 us, profiles/r6/session/point_batch_ab.log)

bool point_eligible(uint64_t seg_bytes, const okv_block_desc* descs, uint32_t nblk, int comp,
                    uint32_t flags) {
  if (comp == OKV_COMP_ZSTD || (flags & OKV_F_INDEX_ONLY) || nblk == 0 ||
      nblk > kPointMaxBlocks || seg_bytes > kPointMaxBytes)
    return false;
  for (uint32_t b = 0; b < nblk; ++b) {
    const Desc& d = reinterpret_cast<const Desc*>(descs)[b];
    if (comp != OKV_COMP_LZ4 && go_read_status(d, seg_bytes) == OKV_BLK_OK &&
        d.block_size > uint64_t(kStage))
      return false;
  }
  return true;
}

// The pinned slab of the point path: at least 1 MiB, so that point reads of
// growing size do not allocate again each time.
int ensure_slab(okv_ctx* ctx, size_t need) {
  return reserve(ctx, ctx->h_slab, std::max<size_t>(need, size_t(1) << 20));
}

// Wait for a point-kernel call by spinning on its completion word in the
// pinned slab (point_done), polling the stream every 1 024 spins so that a
// failed launch ends the wait; hipStreamSynchronize then reports the error.
// (A GetRow is one launch plus this wait; hipStreamSynchronize alone sleeps
// through several microseconds after the kernel's last store.)
int point_wait(okv_ctx* ctx, const volatile uint32_t* done, uint32_t seq) {
  for (uint32_t n = 1; *done != seq; ++n) {
    if ((n & 1023u) == 0 && hipStreamQuery(ctx->stream) != hipErrorNotReady) break;
    __builtin_ia32_pause();
  }
  if (*done != seq) OKV_HIP(hipStreamSynchronize(ctx->stream));
  std::atomic_thread_fence(std::memory_order_acquire);
  return OKV_OK;
}

size_t al(size_t x) { return (x + 255) & ~size_t(255); }  // slab / scratch regions

// One point-kernel call: clear the slab's completion word, launch with the
// next call number (never 0: the cleared word's value) and wait for it.
template <bool kFind>
int point_run(okv_ctx* ctx, const CopyParams& P, Totals* tot, uint32_t* done, const uint8_t* key,
              uint32_t klen, int32_t* found) {
  ctx->last_path = OKV_PATH_POINT;
  *done = 0;
  const uint32_t seq = ++ctx->point_seq ? ctx->point_seq : ++ctx->point_seq;  // (never 0)
  hipLaunchKernelGGL(okv_point_kernel<kFind>, dim3(1), dim3(kThreads), 0, ctx->stream, P, tot,
                     PointFind{key, klen, found, done, seq});
  OKV_HIP(hipGetLastError());
  return point_wait(ctx, done, seq);
}

// One launch, one synchronisation: the blocks and descriptors are copied into
// the pinned slab, the kernel reads them there and writes every output there
// (both over PCIe), and the outputs are copied into the caller's arrays.
int decode_point(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes, const okv_block_desc* descs,
                 uint32_t nblk, int comp, okv_decode_out* o) {
  // output bounds from the descriptors: a readable block's records lie in its
  // BlockSize bytes (>= 6 bytes each); each arena region pads to 16 bytes
  uint64_t R = 0, A = 0;
  for (uint32_t b = 0; b < nblk; ++b) {
    const Desc& d = reinterpret_cast<const Desc*>(descs)[b];
    if (comp == OKV_COMP_LZ4 || go_read_status(d, seg_bytes) != OKV_BLK_OK) continue;
    R += d.block_size / 6;
    A += round16(d.block_size);
  }
  const size_t n1 = size_t(nblk) + 1;
  const size_t o_desc = al(seg_bytes + 64), o_rs = al(o_desc + nblk * sizeof(Desc)),
               o_kb = al(o_rs + n1 * 8), o_vb = al(o_kb + n1 * 8), o_st = al(o_vb + n1 * 8),
               o_tot = al(o_st + n1 * 4), o_ko = al(o_tot + sizeof(Totals) + 16),
               o_kl = al(o_ko + R * 8), o_vo = al(o_kl + R * 2), o_vl = al(o_vo + R * 8),
               o_ka = al(o_vl + R * 4), o_va = al(o_ka + A + 16), total = al(o_va + A + 16);
  int rc = ensure_slab(ctx, total);
  if (rc) return rc;
  uint8_t* S = ctx->h_slab.data();
  if (seg_bytes) std::memcpy(S, seg, seg_bytes);
  std::memcpy(S + o_desc, descs, nblk * sizeof(Desc));
  CopyParams P;
  std::memset(&P, 0, sizeof(P));
  P.seg = S;
  P.seg_bytes = seg_bytes;
  P.descs = reinterpret_cast<const Desc*>(S + o_desc);
  P.nblk = nblk;
  P.comp = comp;
  P.row_start = reinterpret_cast<uint64_t*>(S + o_rs);
  P.key_base = reinterpret_cast<uint64_t*>(S + o_kb);
  P.val_base = reinterpret_cast<uint64_t*>(S + o_vb);
  P.blk_status = reinterpret_cast<int32_t*>(S + o_st);
  P.key_off = reinterpret_cast<uint64_t*>(S + o_ko);
  P.key_len = reinterpret_cast<uint16_t*>(S + o_kl);
  P.val_off = reinterpret_cast<uint64_t*>(S + o_vo);
  P.val_len = reinterpret_cast<uint32_t*>(S + o_vl);
  P.key_arena = S + o_ka;
  P.val_arena = S + o_va;
  P.row_cap = R;
  P.key_cap = A + 16;
  P.val_cap = A + 16;
  Totals* tot = reinterpret_cast<Totals*>(S + o_tot);
  uint32_t* done = reinterpret_cast<uint32_t*>(S + o_tot + sizeof(Totals));
  if ((rc = point_run<false>(ctx, P, tot, done, nullptr, 0, nullptr))) return rc;
  const Totals T = *tot;
  if (!totals_fit(T, false, o))
    return set_err(ctx, OKV_E_CAPACITY, "output capacity too small (totals set)");
  auto out = [](void* dst, const void* src, size_t n) {
    if (dst && n) std::memcpy(dst, src, n);
  };
  out(o->row_start, P.row_start, n1 * 8);
  out(o->blk_status, P.blk_status, size_t(nblk) * 4);
  out(o->key_base, P.key_base, size_t(nblk) * 8);
  out(o->val_base, P.val_base, size_t(nblk) * 8);
  out(o->key_off, P.key_off, T.rows * 8);
  out(o->key_len, P.key_len, T.rows * 2);
  out(o->val_off, P.val_off, T.rows * 8);
  out(o->val_len, P.val_len, T.rows * 4);
  out(o->key_arena, P.key_arena, T.kb);
  out(o->val_arena, P.val_arena, T.vb);
  return OKV_OK;
}

// okv_point_get: GetRow's block step on one block in one launch (the block,
// its descriptor and the key in the pinned slab; the row, if any, back).
int point_get(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes, const okv_block_desc* desc,
              int comp, const uint8_t* key, uint64_t klen, okv_point_row* out) {
  out->status = OKV_BLK_OK;
  out->found = -1;
  out->key = out->val = nullptr;
  out->key_len = out->val_len = 0;
  ctx->last_path = 0;  // (OKV_PATH_POINT once the kernel is launched: okv_last_path)
  if (!ctx->point || klen > kFindKey || !point_eligible(seg_bytes, desc, 1, comp, 0))
    return OKV_OK;  // not a point-path block: the caller decodes it in full
  const Desc& d = *reinterpret_cast<const Desc*>(desc);
  const uint64_t A = go_read_status(d, seg_bytes) == OKV_BLK_OK ? round16(d.block_size) : 0;
  const size_t o_desc = al(seg_bytes + 64), o_key = al(o_desc + sizeof(Desc)),
               o_misc = al(o_key + klen + 16), o_tot = al(o_misc + 72), o_ka = al(o_tot + 64),
               o_va = al(o_ka + A + 16), total = al(o_va + A + 16);
  int rc = ensure_slab(ctx, total);
  if (rc) return rc;
  uint8_t* S = ctx->h_slab.data();
  if (seg_bytes) std::memcpy(S, seg, seg_bytes);
  std::memcpy(S + o_desc, desc, sizeof(Desc));
  if (klen) std::memcpy(S + o_key, key, klen);
  CopyParams P;
  std::memset(&P, 0, sizeof(P));
  P.seg = S;
  P.seg_bytes = seg_bytes;
  P.descs = reinterpret_cast<const Desc*>(S + o_desc);
  P.nblk = 1;
  P.comp = comp;
  uint64_t* misc = reinterpret_cast<uint64_t*>(S + o_misc);  // row_start[2], bases, status, lens
  P.row_start = misc;
  P.key_base = misc + 2;
  P.val_base = misc + 3;
  P.blk_status = reinterpret_cast<int32_t*>(misc + 4);
  P.key_len = reinterpret_cast<uint16_t*>(misc + 5);
  P.val_len = reinterpret_cast<uint32_t*>(misc + 6);
  int32_t* found = reinterpret_cast<int32_t*>(misc + 7);
  P.key_arena = S + o_ka;
  P.val_arena = S + o_va;
  Totals* tot = reinterpret_cast<Totals*>(S + o_tot);
  uint32_t* done = reinterpret_cast<uint32_t*>(misc + 8);
  if ((rc = point_run<true>(ctx, P, tot, done, S + o_key, uint32_t(klen), found))) return rc;
  out->status = *P.blk_status;
  out->found = *found;
  if (out->found == 1) {
    out->key = P.key_arena;
    out->key_len = *P.key_len;
    out->val = P.val_arena;
    out->val_len = *P.val_len;
  }
  return OKV_OK;
}

// Host inputs: the segment and the descriptors into the context's device
// staging buffers (d_seg, d_desc), on the context's stream.
int stage_inputs(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes, const okv_block_desc* descs,
                 uint32_t nblk) {
  int rc;
  if ((rc = reserve(ctx, ctx->d_seg, seg_bytes + 64)) ||
      (rc = reserve(ctx, ctx->d_desc, size_t(nblk) + 2)))
    return rc;
  if (seg_bytes)
    OKV_HIP(hipMemcpyAsync(ctx->d_seg.data(), seg, seg_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (nblk)
    OKV_HIP(hipMemcpyAsync(ctx->d_desc.data(), descs, size_t(nblk) * sizeof(Desc),
                           hipMemcpyHostToDevice, ctx->stream));
  return OKV_OK;
}

// Host pointers: stage inputs to device scratch, decode, copy results back.
// The device outputs are sized from the host descriptors' bounds when those
// exist (one pass-1 walk per call); otherwise from a pass-1 plan first.
int decode_host(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes, const okv_block_desc* descs,
                uint32_t nblk, int comp, okv_decode_out* o, uint32_t flags) {
  if (ctx->point && point_eligible(seg_bytes, descs, nblk, comp, flags))
    return decode_point(ctx, seg, seg_bytes, descs, nblk, comp, o);
  const bool index_only = flags & OKV_F_INDEX_ONLY;
  int rc = stage_inputs(ctx, seg, seg_bytes, descs, nblk);
  if (rc) return rc;
  // device output layout inside one scratch allocation
  const size_t n1 = size_t(nblk) + 1;
  size_t off_rs = 0, off_kb = al(off_rs + n1 * 8), off_vb = al(off_kb + n1 * 8),
         off_st = al(off_vb + n1 * 8), off_rows = al(off_st + n1 * 4);
  uint64_t brows = 0, bbytes = 0;
  const bool bounded = output_bounds(seg, seg_bytes, descs, nblk, comp, uint64_t(1) << 30, &brows,
                                     &bbytes);
  uint64_t R, KB, VB;  // device capacities
  if (bounded) {
    R = std::min<uint64_t>(brows, o->row_cap);
    KB = index_only ? 0 : std::min<uint64_t>(bbytes, o->key_cap);
    VB = index_only ? 0 : std::min<uint64_t>(bbytes, o->val_cap);
  } else {
    rc = reserve(ctx, ctx->d_out, off_rows + 256);
    if (rc) return rc;
    uint8_t* base = ctx->d_out.data();
    Work w;
    rc = prepare(ctx, ctx->d_seg.data(), seg_bytes, ctx->d_desc.data(), nblk, comp, index_only, &w);
    if (rc) return rc;
    if ((rc = ensure_blocks(ctx, nblk))) return rc;
    rc = launch_plan(ctx, w, nblk, reinterpret_cast<uint64_t*>(base + off_rs));
    if (rc) return rc;
    Totals T;
    rc = read_totals(ctx, &T);
    if (rc) return rc;
    if (!totals_fit(T, index_only, o))
      return set_err(ctx, OKV_E_CAPACITY, "output capacity too small (totals set)");
    R = T.rows;
    KB = index_only ? 0 : T.kb;
    VB = index_only ? 0 : T.vb;
  }
  size_t off_ko = al(off_rows), off_kl = al(off_ko + R * 8), off_vo = al(off_kl + R * 2),
         off_vl = al(off_vo + R * 8), off_ka = al(off_vl + R * 4), off_va = al(off_ka + KB),
         total = al(off_va + VB) + 256;
  // grow (keeps nothing: plan results live in ctx scratch, row_start[nblk] is rewritten)
  rc = reserve(ctx, ctx->d_out, total);
  if (rc) return rc;
  uint8_t* base = ctx->d_out.data();
  okv_decode_out d = *o;
  d.row_start = reinterpret_cast<uint64_t*>(base + off_rs);
  d.key_base = reinterpret_cast<uint64_t*>(base + off_kb);
  d.val_base = reinterpret_cast<uint64_t*>(base + off_vb);
  d.blk_status = reinterpret_cast<int32_t*>(base + off_st);
  d.key_off = reinterpret_cast<uint64_t*>(base + off_ko);
  d.key_len = reinterpret_cast<uint16_t*>(base + off_kl);
  d.val_off = reinterpret_cast<uint64_t*>(base + off_vo);
  d.val_len = reinterpret_cast<uint32_t*>(base + off_vl);
  d.key_arena = index_only ? nullptr : base + off_ka;
  d.val_arena = index_only ? nullptr : base + off_va;
  d.row_cap = R;
  d.key_cap = KB;
  d.val_cap = VB;
  rc = decode_device(ctx, ctx->d_seg.data(), seg_bytes, ctx->d_desc.data(), nblk, comp, &d,
                     (flags & ~OKV_F_ASYNC) | OKV_F_DEVICE_PTRS);
  o->n_rows = d.n_rows;
  o->key_bytes = d.key_bytes;
  o->val_bytes = d.val_bytes;
  o->n_bad_blocks = d.n_bad_blocks;
  if (rc) return rc;  // (OKV_E_CAPACITY: the caller's capacity in a bounded decode; totals are set)
  const uint64_t nR = d.n_rows, nK = index_only ? 0 : d.key_bytes, nV = index_only ? 0 : d.val_bytes;
  const size_t nb = index_only ? 0 : size_t(nblk) * 8;  // (no bases, no arenas)
  const struct {
    void* dst;
    const void* src;
    size_t n;
  } copies[] = {{o->row_start, d.row_start, n1 * 8},
                {o->blk_status, d.blk_status, size_t(nblk) * 4},
                {o->key_base, d.key_base, nb},       {o->val_base, d.val_base, nb},
                {o->key_arena, d.key_arena, nK},     {o->val_arena, d.val_arena, nV},
                {o->key_off, d.key_off, nR * 8},     {o->key_len, d.key_len, nR * 2},
                {o->val_off, d.val_off, nR * 8},     {o->val_len, d.val_len, nR * 4}};
  for (const auto& c : copies)
    if (c.dst && c.n)
      OKV_HIP(hipMemcpyAsync(c.dst, c.src, c.n, hipMemcpyDeviceToHost, ctx->stream));
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  return OKV_OK;
}

}  // namespace

extern "C" {

int okv_abi_version(void) { return OKV_ABI_VERSION; }

okv_ctx* okv_open_ex(int device, void* stream, const okv_open_opts* opts) {
  if (opts && opts->size < sizeof(okv_open_opts)) return nullptr;
  okv_ctx* ctx = okv_open_on_stream(device, stream);
  if (ctx && opts) {
    if (opts->flags & OKV_OPEN_NO_FUSED) ctx->fused = false;
    ctx->zstd_one_pass = (opts->flags & OKV_OPEN_ZSTD_ONE_PASS) != 0;
    ctx->point = (opts->flags & OKV_OPEN_NO_POINT) == 0;
  }
  return ctx;
}

okv_ctx* okv_open_on_stream(int device, void* stream) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return nullptr;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  okv_ctx* ctx = new okv_ctx();
  ctx->device = device;
  // Precondition of okv_decode_fused_kernel (see kFusedMaxBlocks): the whole
  // grid is resident at once and dispatched in index order, since each block
  // spins on the look-back words of the blocks before it.  So cap the batch
  // at a quarter of the device's resident capacity for the kernel (room for
  // other contexts' grids on the same device), and at kFusedMaxBlocks.
  {
    int ncu = 0, per_cu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, okv_decode_fused_kernel, 64, 0) !=
            hipSuccess)
      ncu = per_cu = 0;
    ctx->fused_max = std::min<uint32_t>(kFusedMaxBlocks, uint32_t(ncu) * uint32_t(per_cu) / 4);
    if (ctx->fused_max == 0) ctx->fused = false;
  }
#ifdef OKV_ABLATE
  if (!(ctx = ablate_open(ctx))) return nullptr;  // the OKV_* knobs of the alternative forms
#endif
  if (stream) {
    ctx->stream = static_cast<hipStream_t>(stream);
  } else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      delete ctx;
      return nullptr;
    }
    ctx->own_stream = true;
  }
  if (reserve(ctx, ctx->d_tot, 1) || reserve(ctx, ctx->h_tot, 1) || reserve(ctx, ctx->d_span, 1) ||
      reserve(ctx, ctx->h_span, 1)) {
    okv_close(ctx);
    return nullptr;
  }
  return ctx;
}

okv_ctx* okv_open(int device) { return okv_open_on_stream(device, nullptr); }

void okv_close(okv_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  // unchain: contexts that wait on this one, and the one this one waits on
  for (okv_ctx* c : ctx->chained_by)
    if (c->chain == ctx) c->chain = nullptr;
  if (ctx->chain) {
    auto& v = ctx->chain->chained_by;
    v.erase(std::remove(v.begin(), v.end(), ctx), v.end());
  }
  if (ctx->p3_done) (void)hipEventDestroy(ctx->p3_done);
#ifdef OKV_ABLATE
  ablate_close(ctx);  // the arms' second stream and events
#endif
  okv::enc_release(ctx);
  okv::zstd_release(ctx);
  okv::zstd_enc_release(ctx);
  okv::merge_release(ctx);
  okv::get_release(ctx);
  okv::snap_release(ctx);
  okv::range_release(ctx);
  okv::pages_release(ctx);
  const hipStream_t owned = ctx->own_stream ? ctx->stream : nullptr;
  delete ctx;  // every scratch buffer releases itself
  if (owned) (void)hipStreamDestroy(owned);
}

const char* okv_last_error(const okv_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }
void* okv_stream(const okv_ctx* ctx) { return ctx ? ctx->stream : nullptr; }

// Chained contexts are driven from one host thread (as every okv_ctx: not
// thread safe); okv_close unchains both directions, so neither context keeps
// a pointer to a closed one.
int okv_decode_chain(okv_ctx* ctx, okv_ctx* after) {
  if (!ctx || after == ctx || (after && after->device != ctx->device))
    return set_err(ctx, OKV_E_ARG, "okv_decode_chain: contexts");
  int prev = -1;
  OKV_HIP(hipGetDevice(&prev));
  for (okv_ctx* c : {ctx, after}) {
    if (c && !c->p3_done) {
      OKV_HIP(hipSetDevice(c->device));
      const hipError_t e = hipEventCreateWithFlags(&c->p3_done, hipEventDisableTiming);
      if (e != hipSuccess) {
        (void)hipSetDevice(prev);
        return set_err(ctx, OKV_E_HIP, "okv_decode_chain: event", e);
      }
    }
  }
  OKV_HIP(hipSetDevice(prev));  // the caller's current device is left as it was
  if (ctx->chain) {
    auto& v = ctx->chain->chained_by;
    v.erase(std::remove(v.begin(), v.end(), ctx), v.end());
  }
  ctx->chain = after;
  if (after) after->chained_by.push_back(ctx);
  return OKV_OK;
}

int okv_sync(okv_ctx* ctx) {
  if (!ctx) return OKV_E_ARG;
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  return OKV_OK;
}

int okv_decode_plan(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes,
                    const okv_block_desc* descs, uint32_t nblk, int compression, uint32_t flags,
                    uint64_t* n_rows, uint64_t* key_bytes, uint64_t* val_bytes) {
  if (!ctx || (!seg && seg_bytes) || (!descs && nblk)) return set_err(ctx, OKV_E_ARG, "args");
  OKV_HIP(hipSetDevice(ctx->device));
  const uint8_t* d_seg = seg;
  const Desc* d_desc = reinterpret_cast<const Desc*>(descs);
  int rc;
  if (!(flags & OKV_F_DEVICE_PTRS)) {
    if ((rc = stage_inputs(ctx, seg, seg_bytes, descs, nblk))) return rc;
    d_seg = ctx->d_seg.data();
    d_desc = ctx->d_desc.data();
  } else if (!aligned16(seg)) {
    return set_err(ctx, OKV_E_ARG, "device seg must be 16-byte aligned");
  }
  Work w;
  if ((rc = prepare(ctx, d_seg, seg_bytes, d_desc, nblk, compression,
                    (flags & OKV_F_INDEX_ONLY) != 0, &w)))
    return rc;
  OKV_HIP(hipMemsetAsync(ctx->d_span.data(), 0, sizeof(unsigned long long), ctx->stream));
  if ((rc = ensure_blocks(ctx, nblk))) return rc;
  if ((rc = launch_plan(ctx, w, nblk, nullptr, false, nullptr, ~0ull, ctx->d_span.data())))
    return rc;
  OKV_HIP(hipMemcpyAsync(ctx->h_span.data(), ctx->d_span.data(), sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, ctx->stream));
  Totals T;
  if ((rc = read_totals(ctx, &T))) return rc;  // (synchronises: h_span is valid too)
  ctx->span_hint = SpanHint{w.seg, w.descs, w.seg_bytes, nblk, *ctx->h_span};
  if (n_rows) *n_rows = T.rows;
  if (key_bytes) *key_bytes = (flags & OKV_F_INDEX_ONLY) ? 0 : T.kb;
  if (val_bytes) *val_bytes = (flags & OKV_F_INDEX_ONLY) ? 0 : T.vb;
  return OKV_OK;
}

int okv_decode_blocks(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes,
                      const okv_block_desc* descs, uint32_t nblk, int compression,
                      okv_decode_out* out, uint32_t flags) {
  if (!ctx || !out || (!seg && seg_bytes) || (!descs && nblk))
    return set_err(ctx, OKV_E_ARG, "null argument");
  if (compression < 0 || compression > 2) return set_err(ctx, OKV_E_ARG, "compression");
  OKV_HIP(hipSetDevice(ctx->device));
  if (flags & OKV_F_DEVICE_PTRS)
    return decode_device(ctx, seg, seg_bytes, reinterpret_cast<const Desc*>(descs), nblk,
                         compression, out, flags);
  return decode_host(ctx, seg, seg_bytes, descs, nblk, compression, out, flags);
}

int okv_point_get(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes,
                  const okv_block_desc* desc, int compression, const uint8_t* key,
                  uint64_t key_len, okv_point_row* out) {
  if (!ctx || !out || !desc || (!seg && seg_bytes) || (!key && key_len))
    return set_err(ctx, OKV_E_ARG, "null argument");
  if (compression < 0 || compression > 2) return set_err(ctx, OKV_E_ARG, "compression");
  OKV_HIP(hipSetDevice(ctx->device));
  return point_get(ctx, seg, seg_bytes, desc, compression, key, key_len, out);
}

int okv_decode_totals(okv_ctx* ctx, okv_decode_out* out) {
  if (!ctx || !out) return OKV_E_ARG;
  Totals T;
  int rc = read_totals(ctx, &T);
  if (rc) return rc;
  return totals_fit(T, false, out) ? OKV_OK : OKV_E_CAPACITY;
}

int okv_hash_blocks(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes,
                    const okv_block_desc* descs, uint32_t nblk, uint64_t* hashes,
                    uint32_t flags) {
  if (!ctx || !hashes || (!seg && seg_bytes) || (!descs && nblk)) return OKV_E_ARG;
  OKV_HIP(hipSetDevice(ctx->device));
  const uint8_t* d_seg = seg;
  const Desc* d_desc = reinterpret_cast<const Desc*>(descs);
  uint64_t* d_h = hashes;
  int rc;
  if (!(flags & OKV_F_DEVICE_PTRS)) {
    if ((rc = reserve(ctx, ctx->d_hash, size_t(nblk) + 8)) ||
        (rc = stage_inputs(ctx, seg, seg_bytes, descs, nblk)))
      return rc;
    d_seg = ctx->d_seg.data();
    d_desc = ctx->d_desc.data();
    d_h = ctx->d_hash.data();
  }
  if (nblk) {
    launch_hash(ctx->stream, d_seg, seg_bytes, d_desc, nblk, d_h);
    OKV_HIP(hipGetLastError());
  }
  if (nblk && !(flags & OKV_F_DEVICE_PTRS))
    OKV_HIP(hipMemcpyAsync(hashes, d_h, size_t(nblk) * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (!(flags & OKV_F_ASYNC)) OKV_HIP(hipStreamSynchronize(ctx->stream));
  return OKV_OK;
}

uint32_t okv_last_path(const okv_ctx* ctx) { return ctx ? ctx->last_path : 0u; }

int okv_profile(okv_ctx* ctx, int enable) {
  if (!ctx) return OKV_E_ARG;
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  ctx->prof = enable != 0;
  ctx->ev_used = 0;
  for (double& m : ctx->prof_ms) m = 0;
  ctx->prof_calls = 0;
  return OKV_OK;
}

int okv_profile_read(okv_ctx* ctx, double* ms, uint64_t* calls) {
  if (!ctx) return OKV_E_ARG;
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  // intervals: [0,1] zstd stage, [1,2] pass 1, [2,3] pass 2, [3,4] pass 3
  static const int slot[4] = {3, 0, 1, 2};  // -> ms {count, scan, gather, zstd}
  for (size_t i = 0; i + kProfEv <= ctx->ev_used; i += kProfEv) {
    for (int k = 0; k < 4; ++k) {
      float t = 0.f;
      OKV_HIP(hipEventElapsedTime(&t, ctx->ev[i + k], ctx->ev[i + k + 1]));
      ctx->prof_ms[slot[k]] += t;
    }
    ctx->prof_calls++;
  }
  ctx->ev_used = 0;
  if (ms)
    for (int k = 0; k < 4; ++k) ms[k] = ctx->prof_ms[k];
  if (calls) *calls = ctx->prof_calls;
  return OKV_OK;
}

void* okv_device_alloc(okv_ctx* ctx, size_t bytes) {
  void* p = nullptr;
  if (ctx) (void)hipSetDevice(ctx->device);
  if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
  return p;
}
void okv_device_free(okv_ctx* ctx, void* p) {
  if (ctx) (void)hipSetDevice(ctx->device);
  if (p) (void)hipFree(p);
}
void* okv_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, 0) != hipSuccess) return nullptr;
  return p;
}
void okv_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}
int okv_memcpy(okv_ctx* ctx, void* dst, const void* src, size_t bytes, int kind) {
  if (!ctx) return OKV_E_ARG;
  hipMemcpyKind k = kind == 0   ? hipMemcpyHostToDevice
                    : kind == 1 ? hipMemcpyDeviceToHost
                                : hipMemcpyDeviceToDevice;
  OKV_HIP(hipMemcpyAsync(dst, src, bytes, k, ctx->stream));
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  return OKV_OK;
}

}  // extern "C"
