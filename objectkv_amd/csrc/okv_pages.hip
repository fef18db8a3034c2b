// okv_pages.hip -- okv_merge_pages: the Go GetRange loop (snapshot_reader.go:214-372) for
// many small merges ("pages") in one launch.  DESIGN.md 24.
//
// okv_merge_rows is built for one large merge: a dozen launches and three host
// synchronisations, which a page of a thousand rows pays in full.  Here one 256-thread
// workgroup runs a whole page in LDS, in the phases of okv_merge.hip separated by
// workgroup barriers:
//   load     the page, its stream table and the stream offsets
//   prefix   per row the first 16 key bytes and the key length
//   rank     per row its place in the merged order (its index in its stream plus one
//            binary search per other stream over the LDS copy) and whether it owns its
//            key; scattered to merged order at once
//   scan     of the owner flags -> unique keys, and per stream the key it runs out on
//   outcome  per unique key in iteration direction (mrg::go_outcome), scan of the emits,
//            first terminating event (mrg::term_key, an LDS atomicMin)
//   write    the rows, the empty markers of the rest of the slice, the page's counts
// The compare, the outcome and the termination key are okv_merge_kernels.hpp's, shared
// with okv_merge.hip.  No workgroup waits for another, there is no global atomic, and
// every early out is uniform across the workgroup.  Every loop is bounded by the page's
// row count (at most OKV_PAGE_MAX_ROWS), its stream count (at most 64), a key length
// (u16) or its out_cap.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "okv_ctx.hpp"
#include "okv_kernels.hpp"
#include "okv_merge_kernels.hpp"
#include "okv_sst.h"

namespace okv {
namespace pages {

using mrg::Key16;
using mrg::kMaxSrc;
using mrg::Src;

constexpr uint32_t kMaxRows = OKV_PAGE_MAX_ROWS;
constexpr uint32_t kPer = kMaxRows / kThreads;  // flags per thread of a workgroup scan
constexpr uint32_t kEmpty = 0xffffffffu;        // okv_gather_rows' empty row
constexpr uint32_t kMaxCallSrc = 65535;
constexpr uint32_t kGridPages = 1u << 22;       // pages per launch
static_assert(kMaxRows % kThreads == 0, "a workgroup scan covers kPer flags per thread");
static_assert(kMaxRows < 8192, "positions are u16 and a termination key is a u32");

struct Page {  // == okv_page; in the staged image pad carries the host's BIG decision
  uint64_t limit, out_at, out_cap;
  uint32_t src_at, nsrc, bound_at, bound_len, direction, big;
};
static_assert(sizeof(Page) == sizeof(okv_page) && sizeof(Page) == 48, "okv_page layout");

struct Scratch {
  DevBuf<uint8_t> d_img;  // the staged srcs, pages and bounds; host mode: the per-page outputs
  PinBuf<uint8_t> h_img;  // their pinned image
  bool inflight = false;  // an OKV_F_ASYNC call may not have read h_img yet
};

struct Params {
  const Src* srcs;
  const Page* pages;
  const uint8_t* bounds;
  uint32_t page0;  // first page of this launch
  uint32_t* osrc;
  uint64_t* orow;
  uint32_t* n_rows;
  uint32_t* n_unique;
  int32_t* status;
};

namespace {

// Exclusive scan in place of the flags x[0, n) over the workgroup; x[i] for i in
// [n, kMaxRows] becomes the total.  All threads call it, x is complete on entry (a
// barrier before) and on return (a barrier inside).
__device__ __forceinline__ void scan_flags(uint16_t* x, uint32_t n, uint32_t* ws) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t v[kPer], t = 0;
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    const uint32_t i = tid * kPer + u;
    v[u] = i < n ? x[i] : 0;
    t += v[u];
  }
  const uint32_t inc = wave_incl_scan32(t, int(lane));
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  uint32_t run = inc - t;
  for (uint32_t w = 0; w < kThreads / 64; ++w) run += w < wave ? ws[w] : 0;
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    x[tid * kPer + u] = uint16_t(run);
    run += v[u];
  }
  if (tid == kThreads - 1) x[kMaxRows] = uint16_t(run);
  __syncthreads();
}

// src = kEmpty for the slots [from, cap) of the page's slice.
__device__ __forceinline__ void mark_empty(uint32_t* osrc, const Page& pg, uint64_t from) {
  for (uint64_t o = from + threadIdx.x; o < pg.out_cap; o += kThreads) osrc[pg.out_at + o] = kEmpty;
}

__global__ __launch_bounds__(kThreads) void okv_merge_page_kernel(Params P) {
  __shared__ Key16 s_pfx[kMaxRows];         // per row (stream after stream): key prefix
  __shared__ uint16_t s_len[kMaxRows];      // ... key length
  __shared__ uint16_t s_pos[kMaxRows];      // ... merged position; then unique key -> row
  __shared__ uint16_t s_mg[kMaxRows];       // merged order -> row
  __shared__ uint16_t s_own[kMaxRows + 1];  // owner flag in merged order, then its scan
  __shared__ uint8_t s_ev[kMaxRows];        // outcome per unique key, direction order
  __shared__ uint16_t s_emit[kMaxRows + 1]; // emit flags, then their scan
  __shared__ Src s_src[kMaxSrc];
  __shared__ uint64_t s_base[kMaxSrc + 1];  // stream offsets in the row numbering
  __shared__ uint32_t s_end[kMaxSrc];       // per stream: unique key of its last row in direction
  __shared__ uint32_t s_ws[kThreads / 64];
  __shared__ uint32_t s_term;

  const uint32_t tid = threadIdx.x;
  const uint32_t pi = P.page0 + blockIdx.x;
  const Page& pg = P.pages[pi];  // (read where used: a copy held in registers spills SGPRs)
  const uint32_t k = pg.nsrc;  // <= kMaxSrc (the host's check)
  const bool desc = pg.direction == OKV_DIR_DESC;

  // load: the stream table, a word a thread (a Src is 72 bytes: 8-byte aligned, no more)
  {
    static_assert(sizeof(Src) % 8 == 0 && alignof(Src) == 8, "copied as 8-byte words");
    const uint64_t* from = reinterpret_cast<const uint64_t*>(P.srcs + pg.src_at);
    uint64_t* to = reinterpret_cast<uint64_t*>(s_src);
    for (uint32_t t = tid; t < k * uint32_t(sizeof(Src) / 8); t += kThreads) to[t] = from[t];
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t b = 0;
    s_base[0] = 0;
    for (uint32_t j = 0; j < k; ++j) s_base[j + 1] = b += s_src[j].hi - s_src[j].lo;
    s_term = ~0u;
  }
  __syncthreads();
  const uint64_t total = s_base[k];
  if (pg.big || total > kMaxRows || total == 0) {  // (uniform: the same words for every thread)
    mark_empty(P.osrc, pg, 0);
    if (tid == 0) {
      P.n_rows[pi] = 0;
      P.n_unique[pi] = 0;
      P.status[pi] = total == 0 ? 0 : OKV_M_BIG;
    }
    return;
  }
  const uint32_t n = uint32_t(total);

  // A row's key in its stream's arena: read only by a compare that runs past 16 bytes.
  auto key_of = [&](uint32_t j, uint32_t g) {
    const Src& s = s_src[j];
    return s.ka + s.ko[s.lo + (g - s_base[j])];
  };

  // prefix
  for (uint32_t g = tid; g < n; g += kThreads) {
    const uint32_t i = mrg::find_src(s_base, k, g);
    const Src& s = s_src[i];
    const uint64_t r = s.lo + (g - s_base[i]);
    const uint32_t l = s.kl[r];
    s_len[g] = uint16_t(l);
    s_pfx[g] = mrg::be_prefix(s.ka + s.ko[r], l);
    s_mg[g] = 0;  // (input that breaks the header's ordering rule leaves slots unwritten)
    s_own[g] = 0;
  }
  __syncthreads();

  // rank and scatter: earlier streams own ties (count their keys <= key), later ones do not
  for (uint32_t g = tid; g < n; g += kThreads) {
    const uint32_t i = mrg::find_src(s_base, k, g);
    const Key16 p0 = s_pfx[g];
    const uint32_t l0 = s_len[g];
    const uint8_t* k0 = l0 > 16 ? key_of(i, g) : nullptr;
    auto cmp = [&](uint32_t j, uint32_t m) {  // row m of stream j against row g
      const Key16 pm = s_pfx[m];
      const uint32_t lm = s_len[m];
      const bool deep = pm.a == p0.a && pm.b == p0.b && lm > 16 && l0 > 16;
      return mrg::key_cmp(pm, lm, deep ? key_of(j, m) : nullptr, p0, l0, k0);
    };
    uint32_t rank = g - uint32_t(s_base[i]);
    uint32_t owner = 1;
    for (uint32_t j = 0; j < k; ++j) {
      if (j == i) continue;
      const bool le = j < i;
      const uint32_t b0 = uint32_t(s_base[j]);
      uint32_t lo = b0, hi = uint32_t(s_base[j + 1]);
      while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        const int c = cmp(j, m);
        if (c < 0 || (c == 0 && le))
          lo = m + 1;
        else
          hi = m;
      }
      // an earlier stream holding the key owns it: its row lo - 1 equals the key
      if (le && lo > b0 && cmp(j, lo - 1) == 0) owner = 0;
      rank += lo - b0;
    }
    s_pos[g] = uint16_t(rank);  // (< n: every term is at most its stream's rows)
    s_mg[rank] = uint16_t(g);
    s_own[rank] = uint16_t(owner);
  }
  __syncthreads();

  // unique keys
  scan_flags(s_own, n, s_ws);
  const uint32_t nu = s_own[n];
  if (tid < k) {
    uint32_t e = ~0u;  // an empty stream takes no part
    if (s_base[tid + 1] != s_base[tid]) {
      const uint32_t g = uint32_t(desc ? s_base[tid] : s_base[tid + 1] - 1);
      e = uint32_t(s_own[s_pos[g] + 1]) - 1;  // the key's owner is the first row of its run
    }
    s_end[tid] = e;
  }
  __syncthreads();
  for (uint32_t p = tid; p < n; p += kThreads)
    if (s_own[p + 1] != s_own[p]) s_pos[s_own[p]] = s_mg[p];  // s_pos: unique key -> row
  __syncthreads();

  // outcome per unique key, in direction order
  const uint8_t* bound = P.bounds + pg.bound_at;
  const uint32_t blen = pg.bound_len;
  const Key16 bp = mrg::be_prefix(bound, blen);
  for (uint32_t d = tid; d < nu; d += kThreads) {
    const uint32_t u = desc ? nu - 1 - d : d;
    const uint32_t g = s_pos[u];
    const uint32_t i = mrg::find_src(s_base, k, g);
    const Src& s = s_src[i];
    const bool tomb = s.level == 0 && s.vl[s.lo + (g - s_base[i])] == 0;
    // streams that run out on this key; the lowest index is the stale owner
    bool end_here = false;
    uint32_t jmin = k;
    for (uint32_t j = 0; j < k; ++j)
      if (s_end[j] == u) {
        end_here = true;
        jmin = j < jmin ? j : jmin;
      }
    const uint8_t e = mrg::go_outcome(
        tomb, end_here,
        [&] {
          const Key16 pk = s_pfx[g];
          const uint32_t lk = s_len[g];
          const bool deep = pk.a == bp.a && pk.b == bp.b && lk > 16 && blen > 16;
          const int c = mrg::key_cmp(pk, lk, deep ? key_of(i, g) : nullptr, bp, blen, bound);
          return desc ? c <= 0 : c >= 0;
        },
        [&] {
          const Src& t = s_src[jmin];
          return t.level == 0 && t.vl[desc ? t.lo : t.hi - 1] == 0;
        });
    s_ev[d] = e;
    s_emit[d] = e >= mrg::kEmit ? 1 : 0;
  }
  __syncthreads();
  scan_flags(s_emit, nu, s_ws);
  for (uint32_t d = tid; d < nu; d += kThreads) {
    const uint8_t e = s_ev[d];
    const unsigned long long t =
        mrg::term_key(e, d, e >= mrg::kEmit ? uint64_t(s_emit[d]) + 1 : 0, pg.limit);
    if (t != ~0ull) atomicMin(&s_term, uint32_t(t));  // (d + 1 <= kMaxRows: 15 bits)
  }
  __syncthreads();
  uint64_t stop;
  int32_t status;
  mrg::term_decode(s_term == ~0u ? ~0ull : s_term, nu, stop, status);
  const uint32_t nrows = s_emit[stop];  // rows emitted before stop
  if (!status && nrows > pg.out_cap) status = OKV_M_CAPACITY;

  // write
  if (!status)
    for (uint32_t d = tid; d < stop; d += kThreads) {
      if (s_ev[d] < mrg::kEmit) continue;
      const uint32_t g = s_pos[desc ? nu - 1 - d : d];
      const uint32_t i = mrg::find_src(s_base, k, g);
      const uint64_t o = pg.out_at + s_emit[d];
      P.osrc[o] = pg.src_at + i;
      P.orow[o] = s_src[i].lo + (g - s_base[i]);
    }
  mark_empty(P.osrc, pg, status ? 0 : nrows);
  if (tid == 0) {
    P.n_rows[pi] = nrows;
    P.n_unique[pi] = nu;
    P.status[pi] = status;
  }
}

size_t al16(size_t x) { return (x + 15) & ~size_t(15); }

}  // namespace
}  // namespace pages

void pages_release(okv_ctx* ctx) {
  delete ctx->pages;  // the buffers release themselves
  ctx->pages = nullptr;
}

}  // namespace okv

using namespace okv;
using namespace okv::pages;

extern "C" {

int okv_merge_pages(okv_ctx* ctx, const okv_merge_src* srcs, uint32_t nsrc, const okv_page* pgs,
                    uint32_t n_pages, const uint8_t* bounds, uint64_t bounds_len,
                    okv_pages_out* out, uint32_t flags) {
  if (!ctx) return OKV_E_ARG;
  if (!out || (!srcs && nsrc) || (!pgs && n_pages) || (!bounds && bounds_len))
    return set_err(ctx, OKV_E_ARG, "merge_pages: srcs, pages, bounds or out");
  if (nsrc > kMaxCallSrc) return set_err(ctx, OKV_E_ARG, "merge_pages: more than 65535 sources");
  if (n_pages == 0) return OKV_OK;
  if (!out->n_rows || !out->n_unique || !out->status)
    return set_err(ctx, OKV_E_ARG, "merge_pages: a NULL per-page array");
  for (uint32_t s = 0; s < nsrc; ++s)
    if (srcs[s].row_hi < srcs[s].row_lo)
      return set_err(ctx, OKV_E_ARG, "merge_pages: a source with row_hi < row_lo");
  bool slots = false;
  for (uint32_t i = 0; i < n_pages; ++i) {
    const okv_page& p = pgs[i];
    if (p.nsrc > kMaxSrc) return set_err(ctx, OKV_E_ARG, "merge_pages: a page of more than 64 streams");
    if (p.src_at > nsrc || p.nsrc > nsrc - p.src_at)
      return set_err(ctx, OKV_E_ARG, "merge_pages: a page's streams lie outside srcs");
    if (p.limit == 0) return set_err(ctx, OKV_E_ARG, "merge_pages: limit 0");
    if (p.direction != OKV_DIR_ASC && p.direction != OKV_DIR_DESC)
      return set_err(ctx, OKV_E_ARG, "merge_pages: direction");
    if (p.bound_len > 0xffff) return set_err(ctx, OKV_E_ARG, "merge_pages: bound_len > 65535");
    if (uint64_t(p.bound_at) + p.bound_len > bounds_len)
      return set_err(ctx, OKV_E_ARG, "merge_pages: a bound lies outside bounds_len");
    slots |= p.out_cap != 0;
  }
  if (slots && (!out->src || !out->row)) return set_err(ctx, OKV_E_ARG, "merge_pages: src or row");
  OKV_HIP(hipSetDevice(ctx->device));
  if (!ctx->pages) ctx->pages = new Scratch();
  Scratch* sc = ctx->pages;
  hipStream_t st = ctx->stream;
  if (sc->inflight) {  // the last call's copy of the image
    OKV_HIP(hipStreamSynchronize(st));
    sc->inflight = false;
  }
  // one image: srcs, pages, bounds with 16 spare bytes (be_prefix reads the aligned line
  // around a bound), then -- host mode -- room for the three per-page arrays
  const bool dev = flags & OKV_F_DEVICE_PTRS;
  const size_t opg = al16(sizeof(Src) * size_t(nsrc)), obd = opg + sizeof(Page) * size_t(n_pages),
               in_end = al16(obd + bounds_len + 16), end = in_end + (dev ? 0 : 12 * size_t(n_pages));
  int rc;
  if ((rc = reserve(ctx, sc->d_img, end)) || (rc = reserve(ctx, sc->h_img, end))) return rc;
  uint8_t* h = sc->h_img.data();
  uint8_t* b = sc->d_img.data();
  if (nsrc) memcpy(h, srcs, sizeof(Src) * size_t(nsrc));
  memcpy(h + opg, pgs, sizeof(Page) * size_t(n_pages));
  Page* hp = reinterpret_cast<Page*>(h + opg);
  for (uint32_t i = 0; i < n_pages; ++i) {  // BIG is decided here: the host has the ranges
    uint64_t rows = 0;
    for (uint32_t j = 0; j < hp[i].nsrc && rows <= kMaxRows; ++j) {
      const okv_merge_src& s = srcs[hp[i].src_at + j];
      rows += std::min<uint64_t>(s.row_hi - s.row_lo, kMaxRows + 1);
    }
    hp[i].big = rows > kMaxRows;
  }
  if (bounds_len) memcpy(h + obd, bounds, bounds_len);
  memset(h + obd + bounds_len, 0, in_end - (obd + bounds_len));
  OKV_HIP(hipMemcpyAsync(b, h, in_end, hipMemcpyHostToDevice, st));
  Params P;
  memset(&P, 0, sizeof(P));
  P.srcs = reinterpret_cast<const Src*>(b);
  P.pages = reinterpret_cast<const Page*>(b + opg);
  P.bounds = b + obd;
  P.osrc = out->src, P.orow = out->row;
  if (dev) {
    P.n_rows = out->n_rows, P.n_unique = out->n_unique, P.status = out->status;
  } else {
    P.n_rows = reinterpret_cast<uint32_t*>(b + in_end);
    P.n_unique = P.n_rows + n_pages;
    P.status = reinterpret_cast<int32_t*>(P.n_unique + n_pages);
  }
  for (uint32_t at = 0; at < n_pages; at += kGridPages) {
    P.page0 = at;
    hipLaunchKernelGGL(okv_merge_page_kernel, dim3(std::min(n_pages - at, kGridPages)),
                       dim3(kThreads), 0, st, P);
    OKV_HIP(hipGetLastError());
  }
  if (dev) {
    if (flags & OKV_F_ASYNC)
      sc->inflight = true;
    else
      OKV_HIP(hipStreamSynchronize(st));
    return OKV_OK;
  }
  OKV_HIP(hipMemcpyAsync(h + in_end, b + in_end, 12 * size_t(n_pages), hipMemcpyDeviceToHost, st));
  OKV_HIP(hipStreamSynchronize(st));
  memcpy(out->n_rows, h + in_end, 4 * size_t(n_pages));
  memcpy(out->n_unique, h + in_end + 4 * size_t(n_pages), 4 * size_t(n_pages));
  memcpy(out->status, h + in_end + 8 * size_t(n_pages), 4 * size_t(n_pages));
  return OKV_OK;
}

}  // extern "C"
