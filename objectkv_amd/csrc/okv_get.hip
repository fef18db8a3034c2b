// okv_get.hip -- SegmentReader.GetRow (segment_reader.go:362-404) for a batch of keys
// against one segment resident in device memory: the bloom probe, the floor search over
// the block index, ReadBlockWithStat of each touched block once, and the row search,
// one row back per key.  DESIGN.md 20.
//
//   okv_get_locate_kernel   one lane per key: Test(key) (okv_bloom_hash.hpp), then
//                           DescendLessOrEqual over the index image (okv_index.hpp's
//                           floor_upper); a key that lands on a block this path takes
//                           adds 1 to that block's count
//   scan + okv_get_scatter_kernel
//                           the counts scanned exclusively, the keys scattered into
//                           per-block lists, the touched blocks compacted into a work list
//   okv_get_search_kernel   one workgroup per touched block: the block staged into LDS
//                           by LDS DMA, the header walk with Go's checks (walk_staged_to),
//                           then the block's keys spread over the waves, lanes over rows
//   scan + okv_get_values_kernel
//                           round16(val_len) of the found keys scanned in key order, the
//                           values copied out with 16-byte stores
// A zstd segment under OKV_F_GET_ZSTD: between the scatter and the values, the inflate arms
// of okv_get_kernels.hpp instead of the search (okv_get_zplan_kernel, okv_get_zpack_kernel,
// the zstd stage, okv_get_zsearch_kernel, okv_get_zglobal_kernel), then okv_get_zfix_kernel:
// val_off inside the inflated block.  DESIGN.md 25.
//
// The bodies of the locate, scan, scatter, search and value steps are in
// okv_get_kernels.hpp, which okv_snap.hip (the same batch against a whole snapshot) shares.
//
// No kernel waits for another workgroup, and every loop is bounded by an argument of
// the call: the binary search by 64 steps, the probe by k <= 4096, a walk by
// BlockSize / 6 records, a compare by the key length (u16), the lists by the key count.
#include "okv_get_kernels.hpp"

#include <cstring>
#include <memory>

#include "okv_bloom_hash.hpp"

namespace okv {
namespace get {

struct GetTotals {
  uint64_t n_found, n_fallback, val_bytes, blocks;
};

struct Scratch {
  DevBuf<uint32_t> cnt;     // [nt] keys per block (back to zero after the scatter)
  DevBuf<uint64_t> gscan;   // [nt + 1] low word: keys before the block; high: touched blocks
  DevBuf<uint32_t> work;    // [nt] touched blocks (tree positions)
  DevBuf<uint32_t> tpos;    // [n] the key's block (tree position) or kNone
  DevBuf<uint32_t> list;    // [n] keys grouped by block
  DevBuf<uint64_t> vscan;   // [n + 1] exclusive scan of round16(val_len) of found keys
  DevBuf<uint64_t> tsum_in; // scan tile sums
  DevBuf<uint64_t> tsum;    // [tiles + 1] their exclusive scan, then the total
  DevBuf<GetTotals> d_tot;
  PinBuf<GetTotals> h_tot;
  DevBuf<uint8_t> stage;    // host mode: key arrays and per-key outputs
  DevBuf<uint8_t> d_val;    // host mode: the value arena
  ZScratch z;               // the inflate arms (OKV_F_GET_ZSTD)
  bool last_arena = false;  // the last call's arena and capacity (okv_get_totals)
  uint64_t last_cap = 0;
};

struct Params {
  const uint8_t* seg;
  uint64_t seg_bytes;
  int comp;
  const uint8_t* ka;  // keys
  const uint64_t* ko;
  const uint16_t* kl;
  uint32_t n;
  index::View ix;  // index image
  const Desc* descs;
  const uint32_t* file_index;
  const uint64_t* words;  // filter (k == 0: no probe)
  bloom::Modulus mod;
  uint32_t k;
  uint64_t length;
  int32_t* state;  // outputs
  int32_t* blk_status;
  uint32_t* entry;
  uint64_t* val_off;
  uint32_t* val_len;
  uint8_t* val_arena;
  uint64_t val_cap;
  uint32_t* cnt;  // scratch
  uint64_t* gscan;
  uint32_t* work;
  uint32_t* tpos;
  uint32_t* list;
  uint64_t* vscan;
  GetTotals* tot;
  ZView z;  // the inflate arms (z.on: OKV_F_GET_ZSTD on a zstd segment)
};

namespace {

// ---- locate ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void okv_get_locate_kernel(Params P) {
  for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < P.n;
       i += uint64_t(gridDim.x) * kThreads) {
    const uint8_t* key = P.ka + P.ko[i];
    const uint32_t kl = P.kl[i];
    int32_t state, bst;
    uint32_t entry, t;
    locate_key(key, kl, Filter{P.words, P.mod, P.k, P.length}, P.ix, P.descs, P.file_index,
               P.seg_bytes, P.comp, P.z.on != 0, state, bst, entry, t);
    if (t != kNone) atomicAdd(&P.cnt[t], 1u);
    P.state[i] = state;
    P.blk_status[i] = bst;
    P.entry[i] = entry;
    P.val_off[i] = 0;
    P.val_len[i] = 0;
    P.tpos[i] = t;
  }
}

// ---- grouping: keys into per-block lists, touched blocks into the work list ----
__global__ __launch_bounds__(kThreads) void okv_get_scatter_kernel(Params P) {
  scatter_items(P.n, P.ix.nt, P.tpos, P.gscan, P.cnt, P.list, P.work, &P.tot->blocks);
}

// ---- search --------------------------------------------------------------------
struct GetSrc {  // search_blocks over one segment: an item is a key
  const Params& P;
  int32_t* state;
  int32_t* blk_status;
  uint64_t* val_off;
  uint32_t* val_len;
  __device__ __forceinline__ uint32_t touched() const { return uint32_t(P.gscan[P.ix.nt] >> 32); }
  __device__ __forceinline__ bool block(uint32_t w, const uint8_t*& seg, int& comp, Desc& d,
                                        uint32_t& k0, uint32_t& k1) const {
    const uint32_t t = P.work[w];
    seg = P.seg, comp = P.comp, d = P.descs[t];
    k0 = uint32_t(P.gscan[t]), k1 = uint32_t(P.gscan[t + 1]);
    return comp != OKV_COMP_ZSTD;
  }
  __device__ __forceinline__ uint32_t slot(uint32_t w) const { return P.work[w]; }
  __device__ __forceinline__ uint32_t item(uint32_t j) const { return P.list[j]; }
  __device__ __forceinline__ void key(uint32_t i, const uint8_t*& key, uint32_t& kl) const {
    key = P.ka + P.ko[i], kl = P.kl[i];
  }
};

template <uint32_t kCap>
__global__ __launch_bounds__(kSearchThreads) void okv_get_search_kernel(Params P) {
  __shared__ SearchSmem<kCap> sm;
  __shared__ int32_t s_st;
  __shared__ uint32_t s_rows;
  search_blocks<kCap>(GetSrc{P, P.state, P.blk_status, P.val_off, P.val_len}, sm, s_st, s_rows);
}

// ---- the inflate arms (OKV_F_GET_ZSTD) ---------------------------------------------
__global__ __launch_bounds__(kThreads) void okv_get_zplan_kernel(Params P) {
  zplan_blocks(GetSrc{P, P.state, P.blk_status, P.val_off, P.val_len}, P.z);
}
__global__ __launch_bounds__(kThreads) void okv_get_zpack_kernel(Params P) {
  zpack_blocks(GetSrc{P, P.state, P.blk_status, P.val_off, P.val_len}, P.z);
}
template <uint32_t kCap>
__global__ __launch_bounds__(kSearchThreads) void okv_get_zsearch_kernel(Params P) {
  __shared__ SearchSmem<kCap> sm;
  __shared__ int32_t s_st;
  __shared__ uint32_t s_rows;
  const GetSrc src{P, P.state, P.blk_status, P.val_off, P.val_len};
  search_blocks<kCap>(ZSrc<GetSrc>{src, P.z, P.state, P.blk_status, P.val_off, P.val_len}, sm,
                      s_st, s_rows);
}
__global__ __launch_bounds__(kSearchThreads) void okv_get_zglobal_kernel(Params P) {
  __shared__ int32_t s_st;
  __shared__ uint32_t s_rows;
  zglobal_blocks(GetSrc{P, P.state, P.blk_status, P.val_off, P.val_len}, P.z, s_st, s_rows);
}
// One lane per key: a found value's offset into the inflated block (zfix_value).
__global__ __launch_bounds__(kThreads) void okv_get_zfix_kernel(Params P) {
  for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < P.n;
       i += uint64_t(gridDim.x) * kThreads)
    if (P.state[i] == OKV_GET_FOUND) zfix_value(P.z, i, P.tpos[i], P.val_off);
}

// ---- values ----------------------------------------------------------------------
// The totals of the call: found and fallback keys, and the scan's value bytes.
__global__ __launch_bounds__(kThreads) void okv_get_count_kernel(Params P) {
  uint32_t f = 0, fb = 0;
  for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < P.n;
       i += uint64_t(gridDim.x) * kThreads) {
    const int32_t s = P.state[i];
    f += s == OKV_GET_FOUND;
    fb += s == OKV_GET_FALLBACK;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    f += __shfl_xor(f, d, 64);
    fb += __shfl_xor(fb, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (f) atomicAdd(reinterpret_cast<unsigned long long*>(&P.tot->n_found), f);
    if (fb) atomicAdd(reinterpret_cast<unsigned long long*>(&P.tot->n_fallback), fb);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) P.tot->val_bytes = P.vscan[P.n];
}

// One wave per found key: its value from the segment (under the inflate arms: from the
// inflated blocks) into val_arena at the scanned position, 16 bytes a lane, the pad bytes zero.  Nothing is written when the values do
// not fit val_cap.
__global__ __launch_bounds__(kThreads) void okv_get_values_kernel(Params P) {
  if (P.vscan[P.n] > P.val_cap) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t i = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); i < P.n;
       i += waves) {
    if (P.state[i] != OKV_GET_FOUND) continue;
    const uint32_t vl = P.val_len[i];
    uint4* dst = reinterpret_cast<uint4*>(P.val_arena + P.vscan[i]);
    if (P.z.on)
      copy_value(P.z.bytes, P.z.n_bytes, P.z.abs[i], vl, dst, lane);
    else
      copy_value(P.seg, P.seg_bytes, P.val_off[i], vl, dst, lane);
  }
}

// ---- host ------------------------------------------------------------------------
Scratch* scratch(okv_ctx* ctx) {
  if (!ctx->get) ctx->get = new Scratch();
  return ctx->get;
}

// Everything up to the totals, enqueued: locate, grouping, search, the value scan
// (val_pos: where the caller wants the positions, or null) and the counts.
int run(okv_ctx* ctx, Scratch* s, const okv_index* ix, Params& P, uint64_t* val_pos) {
  const uint64_t n = P.n, nt = ix->nt;
  if (int rc = reserve(ctx, s->cnt, size_t(nt))) return rc;
  if (int rc = reserve(ctx, s->gscan, size_t(nt) + 1)) return rc;
  if (int rc = reserve(ctx, s->work, size_t(nt))) return rc;
  if (int rc = reserve(ctx, s->tpos, size_t(n))) return rc;
  if (int rc = reserve(ctx, s->list, size_t(n))) return rc;
  if (int rc = reserve(ctx, s->vscan, size_t(n) + 1)) return rc;
  if (int rc = reserve(ctx, s->d_tot, 1)) return rc;
  if (int rc = reserve(ctx, s->h_tot, 1)) return rc;
  P.cnt = s->cnt.data(), P.gscan = s->gscan.data(), P.work = s->work.data();
  P.tpos = s->tpos.data(), P.list = s->list.data(), P.vscan = s->vscan.data();
  P.tot = s->d_tot.data();
  OKV_HIP(hipMemsetAsync(P.tot, 0, sizeof(GetTotals), ctx->stream));
  if (nt) OKV_HIP(hipMemsetAsync(P.cnt, 0, nt * 4, ctx->stream));
  const uint32_t cap = ix->n_cu * 8;
  const uint32_t gk = std::max(1u, std::min(ceil_div(n, kThreads), cap));
  hipLaunchKernelGGL(okv_get_locate_kernel, dim3(gk), dim3(kThreads), 0, ctx->stream, P);
  OKV_HIP(hipGetLastError());
  const ZKernels<Params> zk{okv_get_zplan_kernel, okv_get_zpack_kernel,
                            okv_get_zsearch_kernel<kSmallCap>,
                            okv_get_zsearch_kernel<uint32_t(kStage)>, okv_get_zglobal_kernel,
                            ix->max_original, false};
  if (P.z.on) {
    if (int rc = reserve(ctx, s->z.abs, size_t(n))) return rc;
    P.z.abs = s->z.abs.data();
  }
  if (nt)
    if (int rc = group_and_search(ctx, s, P, n, nt, ix->max_block, ix->n_cu, okv_get_scatter_kernel,
                                  okv_get_search_kernel<kSmallCap>,
                                  okv_get_search_kernel<uint32_t(kStage)>, P.z.on ? &zk : nullptr))
      return rc;
  if (P.z.on) hipLaunchKernelGGL(okv_get_zfix_kernel, dim3(gk), dim3(kThreads), 0, ctx->stream, P);
  if (int rc = scan(ctx, s->tsum_in, s->tsum, ValLoad{P.state, P.val_len}, n, P.vscan, val_pos)) return rc;
  hipLaunchKernelGGL(okv_get_count_kernel, dim3(gk), dim3(kThreads), 0, ctx->stream, P);
  OKV_HIP(hipGetLastError());
  return OKV_OK;
}

int launch_values(okv_ctx* ctx, const okv_index* ix, const Params& P) {
  const uint32_t g = std::max(1u, std::min(ceil_div(P.n, kThreads / 64), ix->n_cu * 8));
  hipLaunchKernelGGL(okv_get_values_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, P);
  OKV_HIP(hipGetLastError());
  return OKV_OK;
}

int read_totals(okv_ctx* ctx, Scratch* s, okv_get_out* out) {
  OKV_HIP(hipMemcpyAsync(s->h_tot.data(), s->d_tot.data(), sizeof(GetTotals),
                         hipMemcpyDeviceToHost, ctx->stream));
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  out->n_found = s->h_tot->n_found;
  out->n_fallback = s->h_tot->n_fallback;
  out->val_bytes = s->h_tot->val_bytes;
  out->blocks_searched = s->h_tot->blocks;
  return OKV_OK;
}

}  // namespace
}  // namespace get

void get_release(okv_ctx* ctx) {
  delete ctx->get;  // the buffers release themselves
  ctx->get = nullptr;
}

}  // namespace okv

using namespace okv;
using namespace okv::get;

extern "C" {

int okv_index_new(okv_ctx* ctx, const okv_block_desc* descs, const uint8_t* fk_arena,
                  const uint64_t* fk_off, const uint16_t* fk_len, uint64_t n, okv_index** out) {
  if (!ctx || !out) return OKV_E_ARG;
  *out = nullptr;
  if (n && (!descs || !fk_off || !fk_len)) return set_err(ctx, OKV_E_ARG, "index: entries");
  if (n >= kNone) return set_err(ctx, OKV_E_ARG, "index: 2^32 - 1 entries or more");
  for (uint64_t i = 0; i < n; ++i)
    if (fk_len[i] && !fk_arena) return set_err(ctx, OKV_E_ARG, "index: fk_arena");
  OKV_HIP(hipSetDevice(ctx->device));
  const index::Image im = index::build_image(descs, fk_arena, fk_off, fk_len, n);
  std::unique_ptr<okv_index> ix(new okv_index());
  ix->ctx = ctx;
  ix->nt = im.descs.size(), ix->nf = n;
  for (const okv_block_desc& d : im.descs) {
    ix->max_block = std::max(ix->max_block, d.block_size);
    ix->max_original = std::max(ix->max_original, d.original_size);
  }
  ix->n_cu = cu_count(ctx);
  const size_t nt = size_t(ix->nt);
  if (reserve(ctx, ix->descs, nt) || reserve(ctx, ix->file_index, nt) ||
      reserve(ctx, ix->arena, im.arena.size()) || reserve(ctx, ix->off, nt) ||
      reserve(ctx, ix->len, nt) || reserve(ctx, ix->prefix, nt))
    return OKV_E_HIP;
  const hipMemcpyKind h2d = hipMemcpyHostToDevice;
  if (nt) {
    OKV_HIP(hipMemcpyAsync(ix->descs.data(), im.descs.data(), nt * sizeof(Desc), h2d, ctx->stream));
    OKV_HIP(hipMemcpyAsync(ix->file_index.data(), im.file_index.data(), nt * 4, h2d, ctx->stream));
    OKV_HIP(hipMemcpyAsync(ix->off.data(), im.off.data(), nt * 8, h2d, ctx->stream));
    OKV_HIP(hipMemcpyAsync(ix->len.data(), im.len.data(), nt * 2, h2d, ctx->stream));
    OKV_HIP(hipMemcpyAsync(ix->prefix.data(), im.prefix.data(), nt * 8, h2d, ctx->stream));
  }
  if (!im.arena.empty())
    OKV_HIP(hipMemcpyAsync(ix->arena.data(), im.arena.data(), im.arena.size(), h2d, ctx->stream));
  OKV_HIP(hipStreamSynchronize(ctx->stream));  // (the image leaves scope)
  *out = ix.release();
  return OKV_OK;
}

void okv_index_free(okv_index* ix) { delete ix; }  // (the buffers release themselves)

int okv_index_info(const okv_index* ix, uint64_t* n_tree, uint64_t* n_file) {
  if (!ix) return OKV_E_ARG;
  if (n_tree) *n_tree = ix->nt;
  if (n_file) *n_file = ix->nf;
  return OKV_OK;
}

int okv_get_rows(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes, const okv_index* ix,
                 const okv_bloom* bloom, const okv_rows* keys, int compression, okv_get_out* out,
                 uint32_t flags) {
  if (!ctx) return OKV_E_ARG;
  if (!ix || !keys || !out) return set_err(ctx, OKV_E_ARG, "get: index, keys or out");
  if (ix->ctx != ctx) return set_err(ctx, OKV_E_ARG, "get: the index belongs to another context");
  BloomView bv{nullptr, nullptr, 0, 0, 0};
  if (bloom) {
    bv = bloom_view(bloom);
    if (bv.ctx != ctx) return set_err(ctx, OKV_E_ARG, "get: the filter belongs to another context");
    if (bv.k > kMaxK) return set_err(ctx, OKV_E_ARG, "get: bloom k > 4096");
    if (bv.k && bv.m == 0) return set_err(ctx, OKV_E_ARG, "get: bloom m == 0");
  }
  if (compression != OKV_COMP_NONE && compression != OKV_COMP_ZSTD && compression != OKV_COMP_LZ4)
    return set_err(ctx, OKV_E_ARG, "get: compression");
  const uint64_t n = keys->n_rows;
  if (n >= kNone) return set_err(ctx, OKV_E_ARG, "get: 2^32 - 1 keys or more");
  ctx->last_path = 0;
  out->n_found = out->n_fallback = out->val_bytes = out->blocks_searched = 0;
  Scratch* s = scratch(ctx);
  if (int rc = open_call(ctx, s, out, n)) return rc;
  if (n == 0) return OKV_OK;
  if (int rc = key_err(ctx, stage::check_keys(keys, false), "get", "keys")) return rc;
  if (!out->state || !out->blk_status || !out->entry || !out->val_off || !out->val_len)
    return set_err(ctx, OKV_E_ARG, "get: a NULL output array");
  if (!seg && seg_bytes) return set_err(ctx, OKV_E_ARG, "get: seg");
  if (reinterpret_cast<uintptr_t>(seg) & 15)
    return set_err(ctx, OKV_E_ARG, "get: seg is not 16-byte aligned");
  const bool dev = flags & OKV_F_DEVICE_PTRS;
  if (dev && out->val_arena && (reinterpret_cast<uintptr_t>(out->val_arena) & 15))
    return set_err(ctx, OKV_E_ARG, "get: val_arena is not 16-byte aligned");
  OKV_HIP(hipSetDevice(ctx->device));

  Params P;
  memset(&P, 0, sizeof(P));
  P.seg = seg, P.seg_bytes = seg_bytes, P.comp = compression;
  P.n = uint32_t(n);
  P.ix = index::View{ix->prefix.data(), ix->arena.data(), ix->off.data(), ix->len.data(), ix->nt};
  P.descs = ix->descs.data(), P.file_index = ix->file_index.data();
  if (bloom && bv.k) {
    P.words = bv.words, P.mod = bloom::modulus(bv.m), P.k = uint32_t(bv.k), P.length = bv.length;
  }
  P.val_cap = out->val_cap;
  P.z.on = (flags & OKV_F_GET_ZSTD) && compression == OKV_COMP_ZSTD;
  ctx->last_path = OKV_PATH_GET;

  // the per-key arrays: the caller's, or (host mode) staged behind the key arrays
  stage::Col cols[] = {{out->state, 4, false, true},   {out->blk_status, 4, false, true},
                       {out->entry, 4, false, true},   {out->val_off, 8, false, true},
                       {out->val_len, 4, false, true}, {out->val_pos, 8, false, true}};
  KeyRows R;
  if (int rc = stage_keys(ctx, s->stage, keys, dev, "get", "keys", cols, 6, &R)) return rc;
  P.ka = R.ka, P.ko = R.ko, P.kl = R.kl;
  P.state = cols[0].as<int32_t>(), P.blk_status = cols[1].as<int32_t>();
  P.entry = cols[2].as<uint32_t>(), P.val_off = cols[3].as<uint64_t>();
  P.val_len = cols[4].as<uint32_t>();
  if (dev) P.val_arena = out->val_arena;
  if (int rc = run(ctx, s, ix, P, cols[5].as<uint64_t>())) return rc;
  return finish_values(ctx, s, P, out, flags, cols, 6, "get: val_cap too small", read_totals,
                       [&](const Params& p) { return launch_values(ctx, ix, p); });
}

int okv_get_totals(okv_ctx* ctx, okv_get_out* out) {
  if (!ctx || !out) return OKV_E_ARG;
  Scratch* s = ctx->get;
  out->n_found = out->n_fallback = out->val_bytes = out->blocks_searched = 0;
  return last_totals(ctx, s, out, "get: val_cap too small", read_totals);
}

}  // extern "C"
