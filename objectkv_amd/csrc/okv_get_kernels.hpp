// okv_get_kernels.hpp -- the device pieces the batched GetRow of one segment
// (okv_get.hip) and of a snapshot (okv_snap.hip) are both made of: the three-launch
// exclusive scan, the grouping of items by block, the search of a staged block and the
// copy of a value; and the host steps both entry points share: the grouping and search
// launches, the totals, and the values tail of device and host mode (the end of this
// file).  An "item" is what lands on a block: a key (okv_get.hip) or a
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
// when the search takes the block (it is in the segment, not zstd, at most kStage bytes),
// else kNone.
__device__ __forceinline__ void locate_key(const uint8_t* key, uint32_t kl, const Filter& f,
                                           const index::View& ix, const Desc* descs,
                                           const uint32_t* file_index, uint64_t seg_bytes, int comp,
                                           int32_t& state, int32_t& bst, uint32_t& entry,
                                           uint32_t& t) {
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
  bst = go_read_status(d, seg_bytes);  // :303-316, before any read
  if (bst != OKV_BLK_OK)
    state = OKV_GET_BLOCK_ERROR;
  else if (comp == OKV_COMP_ZSTD || d.block_size > uint64_t(kStage))
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
//                                         list[k0 .. k1); it passed go_read_status
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
    src_.block(w, seg, comp, d, k0, k1);
    if (d.block_size > kCap) continue;  // (the launch sized kCap for every block it takes)
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
// The grouping and the search enqueued (nb > 0): cnt scanned over the nb blocks, the n
// items scattered into per-block lists, one workgroup per touched block with the stage
// max_block asks for.
template <class S, class P>
int group_and_search(okv_ctx* ctx, S* s, const P& p, uint64_t n, uint64_t nb, uint64_t max_block,
                     uint32_t n_cu, void (*scatter)(P), void (*search_small)(P),
                     void (*search_large)(P)) {
  if (int rc = scan(ctx, s->tsum_in, s->tsum, CntLoad{p.cnt}, nb, p.gscan, nullptr)) return rc;
  const uint32_t gs = std::max(1u, std::min(ceil_div(std::max(n, nb), kThreads), n_cu * 8));
  hipLaunchKernelGGL(scatter, dim3(gs), dim3(kThreads), 0, ctx->stream, p);
  const bool small = max_block <= kSmallCap;
  const uint64_t most = std::min(n, nb);  // touched blocks at most
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
