// okv_seek.hip -- the two device steps either side of okv_merge_rows when
// snapshot_reader.Reader.GetRange (snapshot_reader.go:208-372) is served from segments
// that stay on the device.  DESIGN.md 23.
//
//   okv_seek_kernel          one lane per (segment, key, direction) triple: the rows
//                            RowIter.Seek + Next yield (okv_seek.hpp's stream)
//   okv_gather_index_kernel  one lane per picked row: its key and value lengths
//   scan x 2                 round16 of those lengths scanned: where each key and value
//                            goes in the packed arenas (okv_get_kernels.hpp's scan)
//   okv_gather_copy_kernel   one wave per picked row: key and value copied with 16-byte
//                            stores, the pad bytes zero (copy_value)
//
// No kernel waits for another workgroup, and every loop is bounded by an argument of the
// call: a search by 64 steps, a compare by the key length (u16), a copy by the row's
// length, the grids by the row count.
#include "okv_get_kernels.hpp"

#include <cstring>

#include "okv_seek.hpp"

namespace okv {
namespace rng {

struct Src {  // == okv_merge_src; the gather reads the six pointers
  const uint8_t* ka;
  const uint64_t* ko;
  const uint16_t* kl;
  const uint8_t* va;
  const uint64_t* vo;
  const uint32_t* vl;
  uint64_t lo, hi;
  int32_t level;
  int32_t pad;
};
static_assert(sizeof(Src) == sizeof(okv_merge_src), "okv_merge_src layout");

constexpr uint32_t kMaxSrc = 65535;

struct Scratch {
  DevBuf<seek::Source> d_seek;  // [nsrc] the seek's sources
  DevBuf<Src> d_src;            // [nsrc] the gather's sources
  DevBuf<uint8_t> stage;        // host mode: the staged inputs and outputs
  PinBuf<uint8_t> h_stage;      // host mode of the seek: their pinned image
  DevBuf<uint8_t> d_key;        // host mode: the arenas
  DevBuf<uint8_t> d_val;
  DevBuf<uint64_t> kscan;       // [n + 1] exclusive scan of round16(key_len)
  DevBuf<uint64_t> vscan;       // [n + 1] ... of round16(val_len)
  DevBuf<uint64_t> tsum_in;     // scan tile sums
  DevBuf<uint64_t> tsum;
  DevBuf<uint64_t> d_tot;       // key_bytes, val_bytes
  PinBuf<uint64_t> h_tot;
};

struct SeekParams {
  const seek::Source* srcs;
  uint32_t nsrc;
  uint32_t n;
  const uint8_t* ka;
  const uint64_t* ko;
  const uint16_t* kl;
  const uint32_t* src_of;
  const uint8_t* direction;
  uint64_t* row_lo;
  uint64_t* row_hi;
};

struct GatherParams {
  const Src* srcs;
  uint32_t nsrc;
  uint32_t n;
  const uint32_t* src;
  const uint64_t* row;
  uint16_t* key_len;
  uint32_t* val_len;
  const uint64_t* kscan;
  const uint64_t* vscan;
  uint8_t* key_arena;
  uint8_t* val_arena;
  uint64_t key_cap, val_cap;
};

namespace {

using get::ceil_div;

__global__ __launch_bounds__(kThreads) void okv_seek_kernel(SeekParams P) {
  const uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= P.n) return;
  uint64_t lo = 0, hi = 0;
  const uint32_t s = P.src_of[i];
  if (s < P.nsrc)
    seek::stream(P.srcs[s], P.ka + P.ko[i], P.kl[i], P.direction[i], lo, hi);
  P.row_lo[i] = lo;
  P.row_hi[i] = hi;
}

__global__ __launch_bounds__(kThreads) void okv_gather_index_kernel(GatherParams P) {
  const uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= P.n) return;
  const uint32_t s = P.src[i];
  const uint64_t r = P.row[i];
  P.key_len[i] = s < P.nsrc ? P.srcs[s].kl[r] : uint16_t(0);
  P.val_len[i] = s < P.nsrc ? P.srcs[s].vl[r] : 0u;
}

struct KeyRoom {  // arena room of row i's key
  const uint16_t* len;
  __device__ uint64_t operator()(uint64_t i) const { return round16(len[i]); }
};
struct ValRoom {
  const uint32_t* len;
  __device__ uint64_t operator()(uint64_t i) const { return round16(len[i]); }
};

// One wave per picked row.  Nothing is written when either arena is too small.  A copy
// reads inside [off, off + len) rounded out to 16-byte lines of the source arena.
__global__ __launch_bounds__(kThreads) void okv_gather_copy_kernel(GatherParams P) {
  if (P.kscan[P.n] > P.key_cap || P.vscan[P.n] > P.val_cap) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t i = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (i >= P.n) return;
  const uint32_t s = P.src[i];
  if (s >= P.nsrc) return;
  const Src& src = P.srcs[s];
  const uint64_t r = P.row[i];
  const uint32_t kl = P.key_len[i], vl = P.val_len[i];
  if (kl) {
    const uint64_t off = src.ko[r];
    get::copy_value(src.ka, off + kl, off, kl, reinterpret_cast<uint4*>(P.key_arena + P.kscan[i]),
                    lane);
  }
  if (vl) {
    const uint64_t off = src.vo[r];
    get::copy_value(src.va, off + vl, off, vl, reinterpret_cast<uint4*>(P.val_arena + P.vscan[i]),
                    lane);
  }
}

__global__ void okv_gather_totals_kernel(const uint64_t* kscan, const uint64_t* vscan,
                                         uint64_t n, uint64_t* tot) {
  tot[0] = kscan[n];
  tot[1] = vscan[n];
}

Scratch* scratch(okv_ctx* ctx) {
  if (!ctx->range) ctx->range = new Scratch();
  return ctx->range;
}

}  // namespace
}  // namespace rng

void range_release(okv_ctx* ctx) {
  delete ctx->range;  // the buffers release themselves
  ctx->range = nullptr;
}

}  // namespace okv

using namespace okv;
using namespace okv::rng;

extern "C" {

int okv_seek_rows(okv_ctx* ctx, const okv_seek_src* srcs, uint32_t nsrc, const okv_rows* keys,
                  const uint32_t* src_of, const uint8_t* direction, uint64_t* row_lo,
                  uint64_t* row_hi, uint32_t flags) {
  if (!ctx) return OKV_E_ARG;
  if (!keys || (!srcs && nsrc)) return set_err(ctx, OKV_E_ARG, "seek: srcs or keys");
  if (nsrc > kMaxSrc) return set_err(ctx, OKV_E_ARG, "seek: more than 65535 sources");
  const uint64_t n = keys->n_rows;
  if (n >= get::kNone) return set_err(ctx, OKV_E_ARG, "seek: 2^32 - 1 triples or more");
  if (n == 0) return OKV_OK;
  if (int rc = key_err(ctx, stage::check_keys(keys, false), "seek", "keys")) return rc;
  if (!src_of || !direction || !row_lo || !row_hi)
    return set_err(ctx, OKV_E_ARG, "seek: a NULL array");
  for (uint32_t s = 0; s < nsrc; ++s)
    if (srcs[s].n_rows && srcs[s].n_blocks &&
        (!srcs[s].key_arena || !srcs[s].key_off || !srcs[s].key_len || !srcs[s].block_first_row))
      return set_err(ctx, OKV_E_ARG, "seek: a source with a NULL array");
  OKV_HIP(hipSetDevice(ctx->device));
  Scratch* sc = scratch(ctx);
  hipStream_t st = ctx->stream;
  const hipMemcpyKind h2d = hipMemcpyHostToDevice, d2h = hipMemcpyDeviceToHost;
  SeekParams P;
  memset(&P, 0, sizeof(P));
  P.nsrc = nsrc, P.n = uint32_t(n);
  const dim3 grid(ceil_div(n, kThreads)), block(kThreads);
  if (flags & OKV_F_DEVICE_PTRS) {
    if (int rc = reserve(ctx, sc->d_seek, std::max<size_t>(nsrc, 1))) return rc;
    // (srcs is pageable memory: the copy has left the caller's array when this returns)
    if (nsrc)
      OKV_HIP(hipMemcpyAsync(sc->d_seek.data(), srcs, sizeof(seek::Source) * nsrc, h2d, st));
    P.srcs = sc->d_seek.data();
    P.ka = keys->key_arena, P.ko = keys->key_off, P.kl = keys->key_len;
    P.src_of = src_of, P.direction = direction, P.row_lo = row_lo, P.row_hi = row_hi;
    hipLaunchKernelGGL(okv_seek_kernel, grid, block, 0, st, P);
    OKV_HIP(hipGetLastError());
    if (!(flags & OKV_F_ASYNC)) OKV_HIP(hipStreamSynchronize(st));
    return OKV_OK;
  }
  if (int rc = key_err(ctx, stage::check_keys(keys, true), "seek", "keys")) return rc;
  for (uint64_t i = 0; i < n; ++i)
    if (src_of[i] >= nsrc) return set_err(ctx, OKV_E_ARG, "seek: src_of names no source");
  // host mode: every input through one pinned image and one copy, both outputs (one
  // column of pairs) back in one.  head: the two arrays not sized by n, one element each
  stage::Col head[] = {{keys->key_arena, keys->key_arena_bytes, true, false},
                       {srcs, sizeof(seek::Source) * nsrc, true, false}};
  stage::Col cols[] = {{keys->key_off, 8, true, false}, {keys->key_len, 2, true, false},
                       {src_of, 4, true, false},        {direction, 1, true, false},
                       {row_lo, 16, false, true}};
  stage::Layout L;
  stage::place(L, head, 2, 1);
  stage::place(L, cols, 5, n);
  int rc;
  if ((rc = reserve(ctx, sc->stage, L.end())) || (rc = reserve(ctx, sc->h_stage, L.end())))
    return rc;
  stage::bind(sc->stage.data(), head, 2);
  stage::bind(sc->stage.data(), cols, 5);
  uint8_t* h = sc->h_stage.data();
  for (const stage::Col& c : head)
    if (c.elem) memcpy(h + c.off, c.host, c.elem);
  for (const stage::Col& c : cols)
    if (c.in) memcpy(h + c.off, c.host, c.elem * n);
  const size_t olo = cols[4].off;
  OKV_HIP(hipMemcpyAsync(sc->stage.data(), h, olo, h2d, st));
  P.ka = head[0].as<const uint8_t>(), P.srcs = head[1].as<const seek::Source>();
  P.ko = cols[0].as<const uint64_t>(), P.kl = cols[1].as<const uint16_t>();
  P.src_of = cols[2].as<const uint32_t>(), P.direction = cols[3].as<const uint8_t>();
  P.row_lo = cols[4].as<uint64_t>(), P.row_hi = P.row_lo + n;
  hipLaunchKernelGGL(okv_seek_kernel, grid, block, 0, st, P);
  OKV_HIP(hipGetLastError());
  OKV_HIP(hipMemcpyAsync(h + olo, P.row_lo, n * 16, d2h, st));
  OKV_HIP(hipStreamSynchronize(st));
  memcpy(row_lo, h + olo, n * 8);
  memcpy(row_hi, h + olo + n * 8, n * 8);
  return OKV_OK;
}

int okv_gather_rows(okv_ctx* ctx, const okv_merge_src* srcs, uint32_t nsrc, const uint32_t* src,
                    const uint64_t* row, uint64_t n, okv_gather_out* out, uint32_t flags) {
  if (!ctx) return OKV_E_ARG;
  if (!out || (!srcs && nsrc)) return set_err(ctx, OKV_E_ARG, "gather: srcs or out");
  if (nsrc > kMaxSrc) return set_err(ctx, OKV_E_ARG, "gather: more than 65535 sources");
  if (n >= get::kNone) return set_err(ctx, OKV_E_ARG, "gather: 2^32 - 1 rows or more");
  if (flags & OKV_F_ASYNC) return set_err(ctx, OKV_E_ARG, "gather: OKV_F_ASYNC");
  out->key_bytes = out->val_bytes = 0;
  if (n == 0) return OKV_OK;
  if (!src || !row) return set_err(ctx, OKV_E_ARG, "gather: src or row");
  if (!out->key_pos || !out->key_len || !out->val_pos || !out->val_len)
    return set_err(ctx, OKV_E_ARG, "gather: a NULL output array");
  if (!out->key_arena != !out->val_arena)
    return set_err(ctx, OKV_E_ARG, "gather: one arena without the other");
  for (uint32_t s = 0; s < nsrc; ++s) {
    if (!srcs[s].key_off || !srcs[s].key_len || !srcs[s].val_off || !srcs[s].val_len)
      return set_err(ctx, OKV_E_ARG, "gather: a source with a NULL array");
    if ((reinterpret_cast<uintptr_t>(srcs[s].key_arena) | reinterpret_cast<uintptr_t>(srcs[s].val_arena)) & 15)
      return set_err(ctx, OKV_E_ARG, "gather: a source arena is not 16-byte aligned");
  }
  const bool dev = flags & OKV_F_DEVICE_PTRS, arenas = out->key_arena != nullptr;
  if (dev && arenas &&
      ((reinterpret_cast<uintptr_t>(out->key_arena) | reinterpret_cast<uintptr_t>(out->val_arena)) & 15))
    return set_err(ctx, OKV_E_ARG, "gather: an output arena is not 16-byte aligned");
  OKV_HIP(hipSetDevice(ctx->device));
  Scratch* sc = scratch(ctx);
  int rc;
  if ((rc = reserve(ctx, sc->d_src, std::max<size_t>(nsrc, 1))) ||
      (rc = reserve(ctx, sc->kscan, size_t(n) + 1)) || (rc = reserve(ctx, sc->vscan, size_t(n) + 1)) ||
      (rc = reserve(ctx, sc->d_tot, 2)) || (rc = reserve(ctx, sc->h_tot, 2)))
    return rc;
  hipStream_t st = ctx->stream;
  const hipMemcpyKind h2d = hipMemcpyHostToDevice, d2h = hipMemcpyDeviceToHost;
  if (nsrc) OKV_HIP(hipMemcpyAsync(sc->d_src.data(), srcs, sizeof(Src) * nsrc, h2d, st));

  GatherParams P;
  memset(&P, 0, sizeof(P));
  P.srcs = sc->d_src.data(), P.nsrc = nsrc, P.n = uint32_t(n);
  P.src = src, P.row = row;
  P.kscan = sc->kscan.data(), P.vscan = sc->vscan.data();
  stage::Col cols[] = {{out->key_pos, 8, false, true}, {out->key_len, 2, false, true},
                       {out->val_pos, 8, false, true}, {out->val_len, 4, false, true}};
  if (dev) {
    stage::direct(cols, 4);
  } else {
    stage::Layout L;
    stage::place(L, cols, 4, n);
    if ((rc = reserve(ctx, sc->stage, L.end()))) return rc;
    stage::bind(sc->stage.data(), cols, 4);
  }
  uint64_t *kpos = cols[0].as<uint64_t>(), *vpos = cols[2].as<uint64_t>();
  P.key_len = cols[1].as<uint16_t>(), P.val_len = cols[3].as<uint32_t>();
  hipLaunchKernelGGL(okv_gather_index_kernel, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, st, P);
  OKV_HIP(hipGetLastError());
  if ((rc = get::scan(ctx, sc->tsum_in, sc->tsum, KeyRoom{P.key_len}, n, sc->kscan.data(), kpos)))
    return rc;
  if ((rc = get::scan(ctx, sc->tsum_in, sc->tsum, ValRoom{P.val_len}, n, sc->vscan.data(), vpos)))
    return rc;
  hipLaunchKernelGGL(okv_gather_totals_kernel, dim3(1), dim3(1), 0, st, sc->kscan.data(),
                     sc->vscan.data(), n, sc->d_tot.data());
  OKV_HIP(hipMemcpyAsync(sc->h_tot.data(), sc->d_tot.data(), 16, d2h, st));
  const dim3 cgrid(ceil_div(n, kThreads / 64)), cblock(kThreads);
  if (dev) {
    if (arenas) {  // (the kernel writes nothing when an arena is too small)
      P.key_arena = out->key_arena, P.val_arena = out->val_arena;
      P.key_cap = out->key_cap, P.val_cap = out->val_cap;
      hipLaunchKernelGGL(okv_gather_copy_kernel, cgrid, cblock, 0, st, P);
      OKV_HIP(hipGetLastError());
    }
    OKV_HIP(hipStreamSynchronize(st));
    out->key_bytes = sc->h_tot.data()[0], out->val_bytes = sc->h_tot.data()[1];
    if (arenas && (out->key_bytes > out->key_cap || out->val_bytes > out->val_cap))
      return set_err(ctx, OKV_E_CAPACITY, "gather: key_cap or val_cap too small");
    return OKV_OK;
  }
  if ((rc = stage_out(ctx, cols, 4, n))) return rc;
  OKV_HIP(hipStreamSynchronize(st));
  out->key_bytes = sc->h_tot.data()[0], out->val_bytes = sc->h_tot.data()[1];
  if (!arenas) return OKV_OK;
  if (out->key_bytes > out->key_cap || out->val_bytes > out->val_cap)
    return set_err(ctx, OKV_E_CAPACITY, "gather: key_cap or val_cap too small");
  if ((rc = reserve(ctx, sc->d_key, std::max<size_t>(size_t(out->key_bytes), 16))) ||
      (rc = reserve(ctx, sc->d_val, std::max<size_t>(size_t(out->val_bytes), 16))))
    return rc;
  P.key_arena = sc->d_key.data(), P.val_arena = sc->d_val.data();
  P.key_cap = out->key_bytes, P.val_cap = out->val_bytes;
  hipLaunchKernelGGL(okv_gather_copy_kernel, cgrid, cblock, 0, st, P);
  OKV_HIP(hipGetLastError());
  if (out->key_bytes)
    OKV_HIP(hipMemcpyAsync(out->key_arena, P.key_arena, out->key_bytes, d2h, st));
  if (out->val_bytes)
    OKV_HIP(hipMemcpyAsync(out->val_arena, P.val_arena, out->val_bytes, d2h, st));
  OKV_HIP(hipStreamSynchronize(st));
  return OKV_OK;
}

}  // extern "C"
