// okv_snap.hip -- snapshot_reader.Reader.GetRow (snapshot_reader.go:104-149) for a batch
// of keys against the segments of a snapshot, all resident in device memory: every
// candidate segment of every key in one pipeline, newest wins.  DESIGN.md 22.
//
//   okv_snap_route_kernel    one lane per key: getPossibleSegmentsForKey over the image
//                            of blockRangeTree (okv_snap_route.hpp's candidates): the
//                            key's run of tree positions and its length
//   scan + okv_snap_emit_kernel
//                            the lengths scanned exclusively; a key's (key, segment)
//                            pairs take consecutive slots
//   okv_snap_locate_kernel   one lane per pair: that segment's bloom probe, floor block
//                            and read status (okv_get_kernels.hpp's locate_key); a pair
//                            that lands on a block this path takes adds 1 to the block's
//                            count.  Blocks are numbered through the whole snapshot.
//   scan + okv_snap_scatter_kernel
//                            pairs into per-block lists, touched blocks into a work list
//   okv_snap_search_kernel   one workgroup per touched block of any segment: the body of
//                            okv_get_search_kernel (search_blocks) over pairs
//   okv_snap_resolve_kernel  one lane per key: its pairs in GetRow's priority order; the
//                            first that is not ErrNoRows decides, later ones stay hidden
//   scan + okv_snap_values_kernel
//                            the values of the found keys, each from its own segment
// Under OKV_F_GET_ZSTD the zstd segments' touched blocks go through the inflate arms of
// okv_get_kernels.hpp behind the scatter (okv_snap_zplan_kernel, okv_snap_zpack_kernel, the
// zstd stage, okv_snap_zsearch_kernel, okv_snap_zglobal_kernel), and okv_snap_zfix_kernel
// behind the resolve turns a found value's offset into one inside its inflated block.
//
// Probing is speculative: a candidate is located and searched even when a newer one
// answers.  No kernel waits for another workgroup, and every loop is bounded by an
// argument of the call or of okv_snap_new: what okv_get.hip lists, the route walk, the
// emit and the resolve by the segment count.
#include "okv_get_kernels.hpp"

#include <cstring>
#include <memory>
#include <vector>

#include "okv_snap_route.hpp"

namespace okv {
namespace snap {

using namespace okv::get;

struct SegDev {  // one segment of the snapshot: device pointers the snapshot does not own
  const uint8_t* seg;
  uint64_t seg_bytes;
  index::View ix;
  const Desc* descs;
  const uint32_t* file_index;
  Filter filter;
  int32_t comp;
  uint32_t level;
  uint32_t block_base;  // the snapshot-wide number of the segment's tree position 0
};

struct SnapTotals {
  uint64_t n_found, n_deleted, n_fallback, val_bytes, pairs, blocks;
};

struct Scratch {
  DevBuf<uint32_t> rlo;     // [n] first tree position of the key's run
  DevBuf<uint32_t> rcnt;    // [n] its length
  DevBuf<uint64_t> pbase;   // [n + 1] pairs before the key; [n]: pairs
  DevBuf<uint32_t> pkey;    // per pair (n * segments slots): its key
  DevBuf<int32_t> pstate;   //   OKV_GET_* of the pair's segment
  DevBuf<int32_t> pbst;
  DevBuf<uint32_t> pentry;
  DevBuf<uint64_t> pvoff;
  DevBuf<uint32_t> pvlen;
  DevBuf<uint32_t> ptpos;   //   the pair's block, numbered through the snapshot, or kNone
  DevBuf<uint32_t> list;    //   pairs grouped by block
  DevBuf<uint32_t> cnt;     // [blocks] pairs per block (back to zero after the scatter)
  DevBuf<uint64_t> gscan;   // [blocks + 1]
  DevBuf<uint32_t> work;    // [blocks] touched blocks
  DevBuf<uint64_t> vscan;   // [n + 1]
  DevBuf<uint64_t> tsum_in, tsum;
  DevBuf<SnapTotals> d_tot;
  PinBuf<SnapTotals> h_tot;
  DevBuf<uint8_t> stage;    // host mode: key arrays and per-key outputs
  DevBuf<uint8_t> d_val;    // host mode: the value arena
  ZScratch z;               // the inflate arms (OKV_F_GET_ZSTD)
  bool last_arena = false;  // the last call's arena and capacity (okv_snap_totals)
  uint64_t last_cap = 0;
};

struct Params {
  const uint8_t* ka;  // keys
  const uint64_t* ko;
  const uint16_t* kl;
  uint32_t n;
  uint32_t ns;  // segments
  uint32_t nb;  // blocks of all segments
  snap_route::View rv;
  const SegDev* segs;       // [ns] tree order
  const uint32_t* by_prio;  // [ns] tree position of priority r
  const uint32_t* blk_seg;  // [nb] the block's segment
  int32_t* state;  // outputs
  uint32_t* seg;
  int32_t* blk_status;
  uint32_t* entry;
  uint64_t* val_off;
  uint32_t* val_len;
  uint8_t* val_arena;
  uint64_t val_cap;
  uint32_t* rlo;  // scratch
  uint32_t* rcnt;
  uint64_t* pbase;
  uint32_t* pkey;
  int32_t* pstate;
  int32_t* pbst;
  uint32_t* pentry;
  uint64_t* pvoff;
  uint32_t* pvlen;
  uint32_t* ptpos;
  uint32_t* list;
  uint32_t* cnt;
  uint64_t* gscan;
  uint32_t* work;
  uint64_t* vscan;
  SnapTotals* tot;
  ZView z;  // the inflate arms (z.on: OKV_F_GET_ZSTD and a zstd segment in the snapshot)
};

namespace {

struct U32Load {
  const uint32_t* v;
  __device__ uint64_t operator()(uint64_t i) const { return v[i]; }
};

// ---- route -------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void okv_snap_route_kernel(Params P) {
  for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < P.n;
       i += uint64_t(gridDim.x) * kThreads) {
    const uint8_t* key = P.ka + P.ko[i];
    const uint32_t kl = P.kl[i];
    uint64_t lo, hi;
    snap_route::candidates(P.rv, key, kl, index::prefix8(key, kl), lo, hi);
    P.rlo[i] = uint32_t(lo);
    P.rcnt[i] = uint32_t(hi - lo);
  }
}

__global__ __launch_bounds__(kThreads) void okv_snap_emit_kernel(Params P) {
  for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < P.n;
       i += uint64_t(gridDim.x) * kThreads) {
    const uint64_t base = P.pbase[i];
    const uint32_t c = min(P.rcnt[i], P.ns);
    for (uint32_t j = 0; j < c; ++j) P.pkey[base + j] = uint32_t(i);
  }
}

// ---- locate ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void okv_snap_locate_kernel(Params P) {
  const uint64_t np = P.pbase[P.n];
  for (uint64_t p = uint64_t(blockIdx.x) * kThreads + threadIdx.x; p < np;
       p += uint64_t(gridDim.x) * kThreads) {
    const uint32_t i = P.pkey[p];
    const SegDev& g = P.segs[P.rlo[i] + uint32_t(p - P.pbase[i])];
    int32_t state, bst;
    uint32_t entry, t;
    locate_key(P.ka + P.ko[i], P.kl[i], g.filter, g.ix, g.descs, g.file_index, g.seg_bytes, g.comp,
               P.z.on != 0, state, bst, entry, t);
    if (t != kNone) {
      t += g.block_base;
      atomicAdd(&P.cnt[t], 1u);
    }
    P.pstate[p] = state;
    P.pbst[p] = bst;
    P.pentry[p] = entry;
    P.pvoff[p] = 0;
    P.pvlen[p] = 0;
    P.ptpos[p] = t;
  }
}

// ---- grouping and search ---------------------------------------------------------
__global__ __launch_bounds__(kThreads) void okv_snap_scatter_kernel(Params P) {
  scatter_items(P.pbase[P.n], P.nb, P.ptpos, P.gscan, P.cnt, P.list, P.work, &P.tot->blocks);
}

struct SnapSrc {  // search_blocks over a snapshot: an item is a (key, segment) pair
  const Params& P;
  int32_t* state;
  int32_t* blk_status;
  uint64_t* val_off;
  uint32_t* val_len;
  __device__ __forceinline__ uint32_t touched() const { return uint32_t(P.gscan[P.nb] >> 32); }
  __device__ __forceinline__ bool block(uint32_t w, const uint8_t*& seg, int& comp, Desc& d,
                                        uint32_t& k0, uint32_t& k1) const {
    const uint32_t b = P.work[w];
    const SegDev& g = P.segs[P.blk_seg[b]];
    seg = g.seg, comp = g.comp, d = g.descs[b - g.block_base];
    k0 = uint32_t(P.gscan[b]), k1 = uint32_t(P.gscan[b + 1]);
    return comp != OKV_COMP_ZSTD;
  }
  __device__ __forceinline__ uint32_t slot(uint32_t w) const { return P.work[w]; }
  __device__ __forceinline__ uint32_t item(uint32_t j) const { return P.list[j]; }
  __device__ __forceinline__ void key(uint32_t p, const uint8_t*& key, uint32_t& kl) const {
    const uint32_t i = P.pkey[p];
    key = P.ka + P.ko[i], kl = P.kl[i];
  }
};

template <uint32_t kCap>
__global__ __launch_bounds__(kSearchThreads) void okv_snap_search_kernel(Params P) {
  __shared__ SearchSmem<kCap> sm;
  __shared__ int32_t s_st;
  __shared__ uint32_t s_rows;
  search_blocks<kCap>(SnapSrc{P, P.pstate, P.pbst, P.pvoff, P.pvlen}, sm, s_st, s_rows);
}

// ---- the inflate arms (OKV_F_GET_ZSTD) ---------------------------------------------
__global__ __launch_bounds__(kThreads) void okv_snap_zplan_kernel(Params P) {
  zplan_blocks(SnapSrc{P, P.pstate, P.pbst, P.pvoff, P.pvlen}, P.z);
}
__global__ __launch_bounds__(kThreads) void okv_snap_zpack_kernel(Params P) {
  zpack_blocks(SnapSrc{P, P.pstate, P.pbst, P.pvoff, P.pvlen}, P.z);
}
template <uint32_t kCap>
__global__ __launch_bounds__(kSearchThreads) void okv_snap_zsearch_kernel(Params P) {
  __shared__ SearchSmem<kCap> sm;
  __shared__ int32_t s_st;
  __shared__ uint32_t s_rows;
  const SnapSrc src{P, P.pstate, P.pbst, P.pvoff, P.pvlen};
  search_blocks<kCap>(ZSrc<SnapSrc>{src, P.z, P.pstate, P.pbst, P.pvoff, P.pvlen}, sm, s_st,
                      s_rows);
}
__global__ __launch_bounds__(kSearchThreads) void okv_snap_zglobal_kernel(Params P) {
  __shared__ int32_t s_st;
  __shared__ uint32_t s_rows;
  zglobal_blocks(SnapSrc{P, P.pstate, P.pbst, P.pvoff, P.pvlen}, P.z, s_st, s_rows);
}
// One lane per key, behind the resolve: the answering pair of a key found in a zstd
// segment names the block (zfix_value).
__global__ __launch_bounds__(kThreads) void okv_snap_zfix_kernel(Params P) {
  for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < P.n;
       i += uint64_t(gridDim.x) * kThreads) {
    if (P.state[i] != OKV_SNAP_FOUND) continue;
    const uint32_t t = P.seg[i];
    if (P.segs[t].comp != OKV_COMP_ZSTD) continue;
    zfix_value(P.z, i, P.ptpos[P.pbase[i] + (t - P.rlo[i])], P.val_off);
  }
}

// ---- resolve -------------------------------------------------------------------
// GetRow's loop (:118-148) over the key's candidates in priority order: ErrNoRows of a
// segment moves on; anything else ends the key, so what a later candidate gave is never
// looked at.  The totals of the call are counted here.
__global__ __launch_bounds__(kThreads) void okv_snap_resolve_kernel(Params P) {
  uint32_t nf = 0, nd = 0, nfb = 0;
  for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < P.n;
       i += uint64_t(gridDim.x) * kThreads) {
    const uint32_t lo = P.rlo[i], c = P.rcnt[i];
    const uint64_t base = P.pbase[i];
    int32_t state = OKV_SNAP_NO_ROWS, bst = OKV_BLK_OK;
    uint32_t seg = kNone, entry = kNone, vlen = 0;
    uint64_t voff = 0;
    uint32_t seen = 0;
    for (uint32_t r = 0; r < P.ns && seen < c; ++r) {
      const uint32_t t = P.by_prio[r];
      if (t - lo >= c) continue;  // (not in [lo, lo + c))
      ++seen;
      const uint64_t p = base + (t - lo);
      const int32_t ps = P.pstate[p];
      if (ps == OKV_GET_BLOOM_NEGATIVE || ps == OKV_GET_NO_BLOCK || ps == OKV_GET_NOT_IN_BLOCK)
        continue;  // ErrNoRows (:122-125)
      seg = t;
      entry = P.pentry[p];
      if (ps == OKV_GET_BLOCK_ERROR) {
        state = OKV_SNAP_SEG_ERROR;
        bst = P.pbst[p];
      } else if (ps == OKV_GET_FALLBACK) {
        state = OKV_SNAP_FALLBACK;
      } else if (P.pvlen[p] == 0 && P.segs[t].level == 0) {
        state = OKV_SNAP_DELETED;  // :136-141
      } else {
        state = OKV_SNAP_FOUND;
        voff = P.pvoff[p];
        vlen = P.pvlen[p];
      }
      break;
    }
    P.state[i] = state;
    P.seg[i] = seg;
    P.blk_status[i] = bst;
    P.entry[i] = entry;
    P.val_off[i] = voff;
    P.val_len[i] = vlen;
    nf += state == OKV_SNAP_FOUND;
    nd += state == OKV_SNAP_DELETED;
    nfb += state == OKV_SNAP_FALLBACK;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    nf += __shfl_xor(nf, d, 64);
    nd += __shfl_xor(nd, d, 64);
    nfb += __shfl_xor(nfb, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (nf) atomicAdd(reinterpret_cast<unsigned long long*>(&P.tot->n_found), nf);
    if (nd) atomicAdd(reinterpret_cast<unsigned long long*>(&P.tot->n_deleted), nd);
    if (nfb) atomicAdd(reinterpret_cast<unsigned long long*>(&P.tot->n_fallback), nfb);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) P.tot->pairs = P.pbase[P.n];
}

// ---- values ----------------------------------------------------------------------
// One wave per found key: its value from its segment (a zstd segment under the inflate
// arms: from the inflated blocks) into val_arena at the scanned position.  Nothing is written when the values do not fit val_cap.
__global__ __launch_bounds__(kThreads) void okv_snap_values_kernel(Params P) {
  if (P.vscan[P.n] > P.val_cap) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t i = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); i < P.n;
       i += waves) {
    if (P.state[i] != OKV_SNAP_FOUND) continue;
    const SegDev& g = P.segs[P.seg[i]];
    uint4* dst = reinterpret_cast<uint4*>(P.val_arena + P.vscan[i]);
    if (P.z.on && g.comp == OKV_COMP_ZSTD)
      copy_value(P.z.bytes, P.z.n_bytes, P.z.abs[i], P.val_len[i], dst, lane);
    else
      copy_value(g.seg, g.seg_bytes, P.val_off[i], P.val_len[i], dst, lane);
  }
}

}  // namespace
}  // namespace snap
}  // namespace okv

struct okv_snap {
  okv_ctx* ctx = nullptr;
  uint32_t ns = 0, nb = 0;
  uint64_t max_block = 0;  // largest BlockSize of any index
  uint64_t max_original = 0;  // largest OriginalSize of a zstd segment's index
  bool zstd = false, plain = false;  // it has zstd segments / segments of another kind
  uint32_t n_cu = 0;
  okv::DevBuf<okv::snap::SegDev> segs;
  okv::DevBuf<uint32_t> by_prio, blk_seg;
  okv::DevBuf<uint8_t> arena;  // the route image
  okv::DevBuf<uint64_t> first_off, last_off, first_prefix, last_prefix;
  okv::DevBuf<uint16_t> first_len, last_len;
};

namespace okv {
namespace snap {
namespace {

static_assert(OKV_SNAP_FOUND == OKV_GET_FOUND, "ValLoad reads either state");

Scratch* scratch(okv_ctx* ctx) {
  if (!ctx->snap) ctx->snap = new Scratch();
  return ctx->snap;
}

// Everything up to the totals, enqueued (val_pos: where the caller wants the positions,
// or null).
int run(okv_ctx* ctx, Scratch* s, const okv_snap* sn, Params& P, uint64_t* val_pos) {
  const uint64_t n = P.n, nb = sn->nb, np_max = n * std::max<uint64_t>(sn->ns, 1);
  if (int rc = reserve(ctx, s->rlo, size_t(n))) return rc;
  if (int rc = reserve(ctx, s->rcnt, size_t(n))) return rc;
  if (int rc = reserve(ctx, s->pbase, size_t(n) + 1)) return rc;
  if (int rc = reserve(ctx, s->pkey, size_t(np_max))) return rc;
  if (int rc = reserve(ctx, s->pstate, size_t(np_max))) return rc;
  if (int rc = reserve(ctx, s->pbst, size_t(np_max))) return rc;
  if (int rc = reserve(ctx, s->pentry, size_t(np_max))) return rc;
  if (int rc = reserve(ctx, s->pvoff, size_t(np_max))) return rc;
  if (int rc = reserve(ctx, s->pvlen, size_t(np_max))) return rc;
  if (int rc = reserve(ctx, s->ptpos, size_t(np_max))) return rc;
  if (int rc = reserve(ctx, s->list, size_t(np_max))) return rc;
  if (int rc = reserve(ctx, s->cnt, size_t(nb))) return rc;
  if (int rc = reserve(ctx, s->gscan, size_t(nb) + 1)) return rc;
  if (int rc = reserve(ctx, s->work, size_t(nb))) return rc;
  if (int rc = reserve(ctx, s->vscan, size_t(n) + 1)) return rc;
  if (int rc = reserve(ctx, s->d_tot, 1)) return rc;
  if (int rc = reserve(ctx, s->h_tot, 1)) return rc;
  P.rlo = s->rlo.data(), P.rcnt = s->rcnt.data(), P.pbase = s->pbase.data();
  P.pkey = s->pkey.data(), P.pstate = s->pstate.data(), P.pbst = s->pbst.data();
  P.pentry = s->pentry.data(), P.pvoff = s->pvoff.data(), P.pvlen = s->pvlen.data();
  P.ptpos = s->ptpos.data(), P.list = s->list.data(), P.cnt = s->cnt.data();
  P.gscan = s->gscan.data(), P.work = s->work.data(), P.vscan = s->vscan.data();
  P.tot = s->d_tot.data();
  OKV_HIP(hipMemsetAsync(P.tot, 0, sizeof(SnapTotals), ctx->stream));
  if (nb) OKV_HIP(hipMemsetAsync(P.cnt, 0, nb * 4, ctx->stream));
  const uint32_t cap = sn->n_cu * 8;
  const uint32_t gk = std::max(1u, std::min(ceil_div(n, kThreads), cap));
  const uint32_t gp = std::max(1u, std::min(ceil_div(np_max, kThreads), cap));
  hipLaunchKernelGGL(okv_snap_route_kernel, dim3(gk), dim3(kThreads), 0, ctx->stream, P);
  OKV_HIP(hipGetLastError());
  if (int rc = scan(ctx, s->tsum_in, s->tsum, U32Load{P.rcnt}, n, P.pbase, nullptr)) return rc;
  if (sn->ns) {
    hipLaunchKernelGGL(okv_snap_emit_kernel, dim3(gk), dim3(kThreads), 0, ctx->stream, P);
    hipLaunchKernelGGL(okv_snap_locate_kernel, dim3(gp), dim3(kThreads), 0, ctx->stream, P);
    OKV_HIP(hipGetLastError());
  }
  const ZKernels<Params> zk{okv_snap_zplan_kernel, okv_snap_zpack_kernel,
                            okv_snap_zsearch_kernel<kSmallCap>,
                            okv_snap_zsearch_kernel<uint32_t(kStage)>, okv_snap_zglobal_kernel,
                            sn->max_original, sn->plain};
  if (P.z.on) {
    if (int rc = reserve(ctx, s->z.abs, size_t(n))) return rc;
    P.z.abs = s->z.abs.data();
  }
  if (nb)
    if (int rc = group_and_search(ctx, s, P, np_max, nb, sn->max_block, sn->n_cu,
                                  okv_snap_scatter_kernel, okv_snap_search_kernel<kSmallCap>,
                                  okv_snap_search_kernel<uint32_t(kStage)>,
                                  P.z.on ? &zk : nullptr))
      return rc;
  hipLaunchKernelGGL(okv_snap_resolve_kernel, dim3(gk), dim3(kThreads), 0, ctx->stream, P);
  if (P.z.on) hipLaunchKernelGGL(okv_snap_zfix_kernel, dim3(gk), dim3(kThreads), 0, ctx->stream, P);
  OKV_HIP(hipGetLastError());
  if (int rc = scan(ctx, s->tsum_in, s->tsum, ValLoad{P.state, P.val_len}, n, P.vscan, val_pos))
    return rc;
  OKV_HIP(hipMemcpyAsync(&P.tot->val_bytes, P.vscan + n, 8, hipMemcpyDeviceToDevice, ctx->stream));
  return OKV_OK;
}

int launch_values(okv_ctx* ctx, const okv_snap* sn, const Params& P) {
  const uint32_t g = std::max(1u, std::min(ceil_div(P.n, kThreads / 64), sn->n_cu * 8));
  hipLaunchKernelGGL(okv_snap_values_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, P);
  OKV_HIP(hipGetLastError());
  return OKV_OK;
}

void zero_totals(okv_snap_out* out) {
  out->n_found = out->n_deleted = out->n_fallback = out->val_bytes = 0;
  out->pairs_probed = out->blocks_searched = 0;
}

int read_totals(okv_ctx* ctx, Scratch* s, okv_snap_out* out) {
  OKV_HIP(hipMemcpyAsync(s->h_tot.data(), s->d_tot.data(), sizeof(SnapTotals),
                         hipMemcpyDeviceToHost, ctx->stream));
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  out->n_found = s->h_tot->n_found;
  out->n_deleted = s->h_tot->n_deleted;
  out->n_fallback = s->h_tot->n_fallback;
  out->val_bytes = s->h_tot->val_bytes;
  out->pairs_probed = s->h_tot->pairs;
  out->blocks_searched = s->h_tot->blocks;
  return OKV_OK;
}

template <class T>
int upload(okv_ctx* ctx, DevBuf<T>& b, const std::vector<T>& v) {
  if (int rc = reserve(ctx, b, v.size())) return rc;
  if (!v.empty())
    OKV_HIP(hipMemcpyAsync(b.data(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice,
                           ctx->stream));
  return OKV_OK;
}

}  // namespace
}  // namespace snap

void snap_release(okv_ctx* ctx) {
  delete ctx->snap;  // the buffers release themselves
  ctx->snap = nullptr;
}

}  // namespace okv

using namespace okv;
using namespace okv::snap;

extern "C" {

int okv_snap_new(okv_ctx* ctx, const okv_snap_seg* segs, uint32_t n_segs, okv_snap** out) {
  if (!ctx || !out) return OKV_E_ARG;
  *out = nullptr;
  if (n_segs && !segs) return set_err(ctx, OKV_E_ARG, "snap: segs");
  snap_route::Image im;
  std::vector<SegDev> sd(n_segs);
  std::vector<uint32_t> by_prio(n_segs, kNone), blk_seg;
  uint64_t nb = 0, max_block = 0, max_original = 0;
  bool has_zstd = false, has_plain = false;
  for (uint32_t i = 0; i < n_segs; ++i) {
    const okv_snap_seg& g = segs[i];
    if (!g.index) return set_err(ctx, OKV_E_ARG, "snap: a segment without an index");
    if (g.index->ctx != ctx)
      return set_err(ctx, OKV_E_ARG, "snap: an index belongs to another context");
    Filter f{nullptr, bloom::Modulus{0, 0}, 0, 0};
    if (g.bloom) {
      const BloomView bv = bloom_view(g.bloom);
      if (bv.ctx != ctx) return set_err(ctx, OKV_E_ARG, "snap: a filter belongs to another context");
      if (bv.k > kMaxK) return set_err(ctx, OKV_E_ARG, "snap: bloom k > 4096");
      if (bv.k && bv.m == 0) return set_err(ctx, OKV_E_ARG, "snap: bloom m == 0");
      if (bv.k) f = Filter{bv.words, bloom::modulus(bv.m), uint32_t(bv.k), bv.length};
    }
    if (g.compression != OKV_COMP_NONE && g.compression != OKV_COMP_ZSTD &&
        g.compression != OKV_COMP_LZ4)
      return set_err(ctx, OKV_E_ARG, "snap: compression");
    if (!g.seg && g.seg_bytes) return set_err(ctx, OKV_E_ARG, "snap: seg");
    if (reinterpret_cast<uintptr_t>(g.seg) & 15)
      return set_err(ctx, OKV_E_ARG, "snap: seg is not 16-byte aligned");
    if ((g.first_len && !g.first_key) || (g.last_len && !g.last_key))
      return set_err(ctx, OKV_E_ARG, "snap: first_key or last_key");
    if (g.priority >= n_segs || by_prio[g.priority] != kNone)
      return set_err(ctx, OKV_E_ARG, "snap: the priorities are not a permutation of 0 .. n_segs - 1");
    by_prio[g.priority] = i;
    const uint8_t none = 0;  // (a key of length 0 may come with a null pointer)
    const uint8_t* fk = g.first_key ? g.first_key : &none;
    if (i && index::compare(fk, g.first_len,
                            im.arena.data() + im.first_off[i - 1], im.first_len[i - 1]) < 0)
      return set_err(ctx, OKV_E_ARG, "snap: segs are not in blockRangeTree order (FirstKey)");
    snap_route::add_record(im, fk, g.first_len, g.last_key ? g.last_key : &none, g.last_len,
                           g.level, g.priority);
    const okv_index* ix = g.index;
    sd[i] = SegDev{g.seg, g.seg_bytes,
                   index::View{ix->prefix.data(), ix->arena.data(), ix->off.data(), ix->len.data(),
                               ix->nt},
                   ix->descs.data(), ix->file_index.data(), f, g.compression, g.level,
                   uint32_t(nb)};
    nb += ix->nt;
    if (nb >= kNone) return set_err(ctx, OKV_E_ARG, "snap: 2^32 - 1 blocks or more");
    blk_seg.insert(blk_seg.end(), size_t(ix->nt), i);
    max_block = std::max(max_block, ix->max_block);
    if (g.compression == OKV_COMP_ZSTD) {
      max_original = std::max(max_original, ix->max_original);
      has_zstd = true;
    } else {
      has_plain = true;
    }
  }
  OKV_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<okv_snap> sn(new okv_snap());
  sn->ctx = ctx;
  sn->ns = n_segs, sn->nb = uint32_t(nb), sn->max_block = max_block;
  sn->max_original = max_original, sn->zstd = has_zstd, sn->plain = has_plain;
  sn->n_cu = cu_count(ctx);
  if (upload(ctx, sn->segs, sd) || upload(ctx, sn->by_prio, by_prio) ||
      upload(ctx, sn->blk_seg, blk_seg) || upload(ctx, sn->arena, im.arena) ||
      upload(ctx, sn->first_off, im.first_off) || upload(ctx, sn->last_off, im.last_off) ||
      upload(ctx, sn->first_prefix, im.first_prefix) ||
      upload(ctx, sn->last_prefix, im.last_prefix) || upload(ctx, sn->first_len, im.first_len) ||
      upload(ctx, sn->last_len, im.last_len))
    return OKV_E_HIP;
  OKV_HIP(hipStreamSynchronize(ctx->stream));  // (the host images leave scope)
  *out = sn.release();
  return OKV_OK;
}

void okv_snap_free(okv_snap* snap) { delete snap; }  // (the buffers release themselves)

int okv_snap_get_rows(okv_ctx* ctx, const okv_snap* sn, const okv_rows* keys, okv_snap_out* out,
                      uint32_t flags) {
  if (!ctx) return OKV_E_ARG;
  if (!sn || !keys || !out) return set_err(ctx, OKV_E_ARG, "snap get: snap, keys or out");
  if (sn->ctx != ctx) return set_err(ctx, OKV_E_ARG, "snap get: the snapshot belongs to another context");
  const uint64_t n = keys->n_rows;
  if (n >= kNone) return set_err(ctx, OKV_E_ARG, "snap get: 2^32 - 1 keys or more");
  if (n * std::max<uint64_t>(sn->ns, 1) >= kNone)
    return set_err(ctx, OKV_E_ARG, "snap get: keys x segments reach 2^32 - 1");
  ctx->last_path = 0;
  zero_totals(out);
  snap::Scratch* s = scratch(ctx);
  if (int rc = open_call(ctx, s, out, n)) return rc;
  if (n == 0) return OKV_OK;
  if (int rc = key_err(ctx, stage::check_keys(keys, false), "snap get", "keys")) return rc;
  if (!out->state || !out->seg || !out->blk_status || !out->entry || !out->val_off || !out->val_len)
    return set_err(ctx, OKV_E_ARG, "snap get: a NULL output array");
  const bool dev = flags & OKV_F_DEVICE_PTRS;
  if (dev && out->val_arena && (reinterpret_cast<uintptr_t>(out->val_arena) & 15))
    return set_err(ctx, OKV_E_ARG, "snap get: val_arena is not 16-byte aligned");
  OKV_HIP(hipSetDevice(ctx->device));

  Params P;
  memset(&P, 0, sizeof(P));
  P.n = uint32_t(n), P.ns = sn->ns, P.nb = sn->nb;
  P.rv = snap_route::View{index::View{sn->first_prefix.data(), sn->arena.data(),
                                      sn->first_off.data(), sn->first_len.data(), sn->ns},
                          sn->last_prefix.data(), sn->last_off.data(), sn->last_len.data()};
  P.segs = sn->segs.data(), P.by_prio = sn->by_prio.data(), P.blk_seg = sn->blk_seg.data();
  P.val_cap = out->val_cap;
  P.z.on = (flags & OKV_F_GET_ZSTD) && sn->zstd;
  ctx->last_path = OKV_PATH_SNAP_GET;

  // the per-key arrays: the caller's, or (host mode) staged behind the key arrays
  stage::Col cols[] = {{out->state, 4, false, true},      {out->seg, 4, false, true},
                       {out->blk_status, 4, false, true}, {out->entry, 4, false, true},
                       {out->val_off, 8, false, true},    {out->val_len, 4, false, true},
                       {out->val_pos, 8, false, true}};
  KeyRows R;
  if (int rc = stage_keys(ctx, s->stage, keys, dev, "snap get", "keys", cols, 7, &R)) return rc;
  P.ka = R.ka, P.ko = R.ko, P.kl = R.kl;
  P.state = cols[0].as<int32_t>(), P.seg = cols[1].as<uint32_t>();
  P.blk_status = cols[2].as<int32_t>(), P.entry = cols[3].as<uint32_t>();
  P.val_off = cols[4].as<uint64_t>(), P.val_len = cols[5].as<uint32_t>();
  if (dev) P.val_arena = out->val_arena;
  if (int rc = run(ctx, s, sn, P, cols[6].as<uint64_t>())) return rc;
  return finish_values(ctx, s, P, out, flags, cols, 7, "snap get: val_cap too small", read_totals,
                       [&](const Params& p) { return launch_values(ctx, sn, p); });
}

int okv_snap_totals(okv_ctx* ctx, okv_snap_out* out) {
  if (!ctx || !out) return OKV_E_ARG;
  snap::Scratch* s = ctx->snap;
  zero_totals(out);
  return last_totals(ctx, s, out, "snap get: val_cap too small", read_totals);
}

}  // extern "C"
