// okv_bloom.hip -- bloom.BloomFilter (bits-and-blooms v2.0.3) resident on the device:
// Add(key) for every row of an okv_rows, the batched Test, and WriteTo's bytes, so a
// default-options segment (segment_writer_option.go:20; WriteRow :133-136,
// generateMetaBlock :295-300) can be written from rows that never visit the host.
// The arithmetic is okv_bloom_hash.hpp's, the form the host test program checks.
// DESIGN.md 19.
//
// A filter is wordsNeeded(length) uint64 words in device memory (native little-endian
// words; WriteTo swaps them) plus m, k and length on the host side of the handle.
// Every kernel is sized from m, k and the row count alone, k is capped at kMaxK, and
// no workgroup waits for another.
#include "okv_ctx.hpp"

#include <cmath>
#include <cstring>

#include "okv_bloom_hash.hpp"
#include "okv_stage.hpp"

struct okv_bloom {
  okv_ctx* ctx = nullptr;
  uint64_t m = 0, k = 0, length = 0;
  uint64_t words = 0;                       // wordsNeeded(length)
  okv::DevBuf<uint64_t> bits;               // [words]
  uint32_t n_cu = 0;
  // scratch of the host-mode calls (a const filter still stages through them)
  mutable uint32_t last_path = 0;           // OKV_BLOOM_PATH_* of the last add
  mutable okv::DevBuf<uint8_t> stage;       // key arena, offsets, lengths, probe results
  mutable okv::PinBuf<uint8_t> pin;         // WriteTo bytes for a host destination
};

namespace okv {
namespace {

constexpr uint32_t kLdsThreads = 1024;      // one workgroup per CU: 4 waves per SIMD
constexpr uint32_t kSliceShift = 20;        // bits of the filter per LDS slice: 128 KiB
constexpr uint32_t kSliceBits = 1u << kSliceShift;
constexpr uint32_t kSliceWords = kSliceBits / 64;
constexpr uint64_t kMaxLdsWords = (1ull << 20) / 8;  // the LDS form: filters of up to 1 MiB
constexpr uint64_t kMaxK = 4096;            // documented divergence: Go has no cap
// automatic form: below this many locations (rows x k) a call takes the global form.
// Measured on the default filter (3 slices, k = 20): global 21.9 us against LDS 24.7 at
// 16 384 rows, 33.0 against 29.2 at 32 768, 82.4 against 47.1 at 100 000; the difference
// changes sign near 23 000 rows = 4.7e5 locations
constexpr uint64_t kLdsMinLocations = 1ull << 19;

// Add, LDS-sliced form.  Workgroup b accumulates slice b % S of the bit array
// (2^20 bits) in LDS over the rows of group b / S, then ORs its non-zero words into
// the global words once.  Hashes are recomputed per slice.
__global__ __launch_bounds__(kLdsThreads) void okv_bloom_add_lds_kernel(
    KeyRows R, uint64_t* __restrict__ words, uint64_t nwords, bloom::Modulus mod, uint32_t k,
    uint32_t S) {
  __shared__ uint32_t lds[kSliceBits / 32];
  const uint32_t slice = blockIdx.x % S, group = blockIdx.x / S, groups = gridDim.x / S;
  const uint64_t w_lo = uint64_t(slice) * kSliceWords;
  const uint32_t nw = uint32_t(min(nwords - w_lo, uint64_t(kSliceWords)));  // (w_lo < nwords)
  for (uint32_t i = threadIdx.x; i < 2 * nw; i += kLdsThreads) lds[i] = 0;
  __syncthreads();
  for (uint64_t row = uint64_t(group) * kLdsThreads + threadIdx.x; row < R.n;
       row += uint64_t(groups) * kLdsThreads) {
    uint64_t h[4];
    bloom::base_hashes(R.ka + R.ko[row], R.kl[row], h);
    for (uint32_t i = 0; i < k; ++i) {
      const uint64_t loc = bloom::location(h, i, mod);  // < m <= 64 nwords
      if ((loc >> kSliceShift) == slice) {
        const uint32_t b = uint32_t(loc) & (kSliceBits - 1);
        atomicOr(&lds[b >> 5], 1u << (b & 31));
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nw; i += kLdsThreads) {
    const uint64_t v = uint64_t(lds[2 * i]) | (uint64_t(lds[2 * i + 1]) << 32);
    if (v) atomicOr(reinterpret_cast<unsigned long long*>(words + w_lo + i), v);
  }
}

// Add, global form: one no-return device-scope atomic OR per location.
__global__ __launch_bounds__(kThreads) void okv_bloom_add_global_kernel(
    KeyRows R, uint64_t* __restrict__ words, bloom::Modulus mod, uint32_t k) {
  for (uint64_t row = uint64_t(blockIdx.x) * kThreads + threadIdx.x; row < R.n;
       row += uint64_t(gridDim.x) * kThreads) {
    uint64_t h[4];
    bloom::base_hashes(R.ka + R.ko[row], R.kl[row], h);
    for (uint32_t i = 0; i < k; ++i) {
      const uint64_t loc = bloom::location(h, i, mod);
      atomicOr(reinterpret_cast<unsigned long long*>(words + (loc >> 6)), 1ull << (loc & 63));
    }
  }
}

// Test: up to k probes per key; a location >= length reads as unset (bitset.Test).
__global__ __launch_bounds__(kThreads) void okv_bloom_test_kernel(
    KeyRows R, const uint64_t* __restrict__ words, bloom::Modulus mod, uint32_t k,
    uint64_t length, uint8_t* __restrict__ maybe) {
  for (uint64_t row = uint64_t(blockIdx.x) * kThreads + threadIdx.x; row < R.n;
       row += uint64_t(gridDim.x) * kThreads) {
    uint64_t h[4];
    bloom::base_hashes(R.ka + R.ko[row], R.kl[row], h);
    uint8_t r = 1;
    for (uint32_t i = 0; i < k; ++i) {
      const uint64_t loc = bloom::location(h, i, mod);
      if (loc >= length || !((words[loc >> 6] >> (loc & 63)) & 1)) {
        r = 0;
        break;
      }
    }
    maybe[row] = r;
  }
}

// WriteTo: big-endian m, k, length, then the words (dst is 8-byte aligned).
__global__ __launch_bounds__(kThreads) void okv_bloom_write_kernel(
    const uint64_t* __restrict__ words, uint64_t nwords, uint64_t m, uint64_t k, uint64_t length,
    uint64_t* __restrict__ dst) {
  for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < nwords + 3;
       i += uint64_t(gridDim.x) * kThreads) {
    const uint64_t v = i == 0 ? m : i == 1 ? k : i == 2 ? length : words[i - 3];
    dst[i] = __builtin_bswap64(v);
  }
}

uint64_t words_needed(uint64_t length) {  // bitset.wordsNeeded, with its overflow guard
  const uint64_t cap = ~uint64_t(0);
  return length > cap - 64 + 1 ? cap >> 6 : (length + 63) >> 6;
}

uint32_t grid_for(const okv_bloom* f, uint64_t n) {
  return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>((n + kThreads - 1) / kThreads,
                                                            uint64_t(f->n_cu) * 8)));
}

int make_filter(okv_ctx* ctx, uint64_t m, uint64_t k, uint64_t length, okv_bloom** out) {
  okv_bloom* f = new okv_bloom();
  f->ctx = ctx;
  f->m = m, f->k = k, f->length = length;
  f->words = words_needed(length);
  f->n_cu = cu_count(ctx);
  if (f->words > (uint64_t(1) << 40)) {  // 8 TiB of words: not a device allocation
    delete f;
    return set_err(ctx, OKV_E_NOMEM, "bloom: filter too large");
  }
  if (int rc = reserve(ctx, f->bits, size_t(f->words))) {
    delete f;
    return rc;
  }
  *out = f;
  return OKV_OK;
}

int own(okv_ctx* ctx, const okv_bloom* f) {
  if (!ctx || !f) return OKV_E_ARG;
  if (f->ctx != ctx) return set_err(ctx, OKV_E_ARG, "bloom: the filter belongs to another context");
  return OKV_OK;
}

}  // namespace

BloomView bloom_view(const okv_bloom* f) {
  return BloomView{f->ctx, f->bits.data(), f->m, f->k, f->length};
}

}  // namespace okv

using namespace okv;

extern "C" {

// bloom.EstimateParameters
void okv_bloom_estimate(uint64_t n, double p, uint64_t* m, uint64_t* k) {
  const double mm = std::ceil(-1 * double(n) * std::log(p) / std::pow(std::log(2.0), 2));
  const double kk = std::ceil(std::log(2.0) * mm / double(n));
  if (m) *m = uint64_t(mm);
  if (k) *k = uint64_t(kk);
}

int okv_bloom_new(okv_ctx* ctx, uint64_t m, uint64_t k, okv_bloom** out) {
  if (!ctx || !out) return OKV_E_ARG;
  *out = nullptr;
  OKV_HIP(hipSetDevice(ctx->device));
  m = std::max<uint64_t>(1, m), k = std::max<uint64_t>(1, k);
  okv_bloom* f;
  if (int rc = make_filter(ctx, m, k, m, &f)) return rc;
  const hipError_t e = hipMemsetAsync(f->bits.data(), 0, f->words * 8, ctx->stream);
  if (e != hipSuccess) {
    delete f;
    return set_err(ctx, OKV_E_HIP, "bloom: zeroing the filter", e);
  }
  *out = f;
  return OKV_OK;
}

// BloomFilter.ReadFrom, by the rules of bloom_read_from (okv_host.cpp): big-endian m,
// k, bitset length, then wordsNeeded(length) words; a short input is an error,
// trailing bytes are not read.
int okv_bloom_read_from(okv_ctx* ctx, const uint8_t* b, uint64_t len, okv_bloom** out) {
  if (!ctx || !out) return OKV_E_ARG;
  *out = nullptr;
  if (!b || len < 24) return set_err(ctx, OKV_E_ARG, "bloom ReadFrom: unexpected EOF");
  const auto be64 = [](const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return __builtin_bswap64(v);
  };
  const uint64_t m = be64(b), k = be64(b + 8), length = be64(b + 16);
  const uint64_t words = words_needed(length);
  if (words > (len - 24) / 8) return set_err(ctx, OKV_E_ARG, "bloom ReadFrom: too few words");
  OKV_HIP(hipSetDevice(ctx->device));
  okv_bloom* f;
  if (int rc = make_filter(ctx, m, k, length, &f)) return rc;
  std::vector<uint64_t> w(size_t(words) ? size_t(words) : 1);
  for (uint64_t i = 0; i < words; ++i) w[size_t(i)] = be64(b + 24 + 8 * i);
  hipError_t e = hipMemcpyAsync(f->bits.data(), w.data(), words * 8, hipMemcpyHostToDevice,
                                ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (w leaves scope)
  if (e != hipSuccess) {
    delete f;
    return set_err(ctx, OKV_E_HIP, "bloom ReadFrom: upload", e);
  }
  *out = f;
  return OKV_OK;
}

void okv_bloom_free(okv_bloom* f) { delete f; }  // (the buffers release themselves)

int okv_bloom_info(const okv_bloom* f, uint64_t* m, uint64_t* k, uint64_t* length,
                   uint64_t* write_to_bytes) {
  if (!f) return OKV_E_ARG;
  if (m) *m = f->m;
  if (k) *k = f->k;
  if (length) *length = f->length;
  if (write_to_bytes) *write_to_bytes = 24 + 8 * f->words;
  return OKV_OK;
}

// ClearAll: enqueued on the context stream, like every other change of the words.
int okv_bloom_clear(okv_ctx* ctx, okv_bloom* f) {
  if (int rc = own(ctx, f)) return rc;
  OKV_HIP(hipSetDevice(ctx->device));
  OKV_HIP(hipMemsetAsync(f->bits.data(), 0, f->words * 8, ctx->stream));
  return OKV_OK;
}

int okv_bloom_add_rows(okv_ctx* ctx, okv_bloom* f, const okv_rows* rows, uint32_t flags) {
  if (int rc = own(ctx, f)) return rc;
  if (!rows) return set_err(ctx, OKV_E_ARG, "bloom: rows");
  if ((flags & OKV_BLOOM_FORCE_LDS) && (flags & OKV_BLOOM_FORCE_GLOBAL))
    return set_err(ctx, OKV_E_ARG, "bloom: both forms forced");
  // Go's bitset.Set would grow a set shorter than m; m == 0 is its division panic
  if (f->length != f->m || f->m == 0)
    return set_err(ctx, OKV_E_ARG, "bloom Add: bitset length != m");
  if (f->k > kMaxK) return set_err(ctx, OKV_E_ARG, "bloom: k > 4096");
  const bool lds_fits = f->words <= kMaxLdsWords;
  if ((flags & OKV_BLOOM_FORCE_LDS) && !lds_fits)
    return set_err(ctx, OKV_E_ARG, "bloom: the LDS form takes filters of up to 1 MiB");
  f->last_path = 0;
  const uint64_t n = rows->n_rows;
  if (n == 0) return OKV_OK;
  OKV_HIP(hipSetDevice(ctx->device));
  const bool dev = flags & OKV_F_DEVICE_PTRS;
  KeyRows R;
  if (int rc = stage_keys(ctx, f->stage, rows, dev, "bloom", "rows", nullptr, 0, &R)) return rc;
  const bool lds = (flags & OKV_BLOOM_FORCE_LDS) ||
                   (!(flags & OKV_BLOOM_FORCE_GLOBAL) && lds_fits && n * f->k >= kLdsMinLocations);
  const bloom::Modulus mod = bloom::modulus(f->m);
  if (lds) {
    const uint32_t S = uint32_t((f->words + kSliceWords - 1) / kSliceWords);  // 1..8
    const uint32_t G = uint32_t(std::max<uint64_t>(
        1, std::min<uint64_t>((n + kLdsThreads - 1) / kLdsThreads, f->n_cu / S)));
    hipLaunchKernelGGL(okv_bloom_add_lds_kernel, dim3(S * G), dim3(kLdsThreads), 0, ctx->stream, R,
                       f->bits.data(), f->words, mod, uint32_t(f->k), S);
  } else {
    hipLaunchKernelGGL(okv_bloom_add_global_kernel, dim3(grid_for(f, n)), dim3(kThreads), 0,
                       ctx->stream, R, f->bits.data(), mod, uint32_t(f->k));
  }
  OKV_HIP(hipGetLastError());
  f->last_path = lds ? OKV_BLOOM_PATH_LDS : OKV_BLOOM_PATH_GLOBAL;
  if (!dev || !(flags & OKV_F_ASYNC)) OKV_HIP(hipStreamSynchronize(ctx->stream));
  return OKV_OK;
}

int okv_bloom_test_rows(okv_ctx* ctx, const okv_bloom* f, const okv_rows* rows, uint8_t* maybe,
                        uint32_t flags) {
  if (int rc = own(ctx, f)) return rc;
  if (!rows) return set_err(ctx, OKV_E_ARG, "bloom: rows");
  const uint64_t n = rows->n_rows;
  if (n && !maybe) return set_err(ctx, OKV_E_ARG, "bloom Test: maybe");
  if (f->k > kMaxK) return set_err(ctx, OKV_E_ARG, "bloom: k > 4096");
  if (f->k && f->m == 0)  // Go's integer-division panic (the host probe: OKV_R_PANIC)
    return set_err(ctx, OKV_E_ARG, "bloom Test: m == 0");
  if (n == 0) return OKV_OK;
  OKV_HIP(hipSetDevice(ctx->device));
  const bool dev = flags & OKV_F_DEVICE_PTRS;
  if (f->k == 0) {  // no probe fails
    if (dev)
      OKV_HIP(hipMemsetAsync(maybe, 1, n, ctx->stream));
    else
      memset(maybe, 1, n);
  } else {
    KeyRows R;
    stage::Col m{maybe, 1, false, true};
    if (int rc = stage_keys(ctx, f->stage, rows, dev, "bloom", "rows", &m, 1, &R)) return rc;
    hipLaunchKernelGGL(okv_bloom_test_kernel, dim3(grid_for(f, n)), dim3(kThreads), 0, ctx->stream,
                       R, f->bits.data(), bloom::modulus(f->m), uint32_t(f->k), f->length,
                       m.as<uint8_t>());
    OKV_HIP(hipGetLastError());
    if (!dev)
      if (int rc = stage_out(ctx, &m, 1, n)) return rc;
  }
  if (!dev || !(flags & OKV_F_ASYNC)) OKV_HIP(hipStreamSynchronize(ctx->stream));
  return OKV_OK;
}

int okv_bloom_write_to(okv_ctx* ctx, const okv_bloom* f, uint8_t* dst, uint64_t cap,
                       uint32_t flags) {
  if (int rc = own(ctx, f)) return rc;
  if (!dst) return set_err(ctx, OKV_E_ARG, "bloom WriteTo: dst");
  const uint64_t need = 24 + 8 * f->words;
  if (cap < need) return set_err(ctx, OKV_E_CAPACITY, "bloom WriteTo: cap too small");
  const bool dev = flags & OKV_F_DEVICE_PTRS;
  if (dev && (reinterpret_cast<uintptr_t>(dst) & 7))
    return set_err(ctx, OKV_E_ARG, "bloom WriteTo: device dst is not 8-byte aligned");
  OKV_HIP(hipSetDevice(ctx->device));
  uint64_t* out = reinterpret_cast<uint64_t*>(dst);
  if (!dev) {  // the kernel writes the pinned buffer; the bytes are copied out after it
    if (int rc = reserve(ctx, f->pin, size_t(need))) return rc;
    out = reinterpret_cast<uint64_t*>(f->pin.data());
  }
  hipLaunchKernelGGL(okv_bloom_write_kernel, dim3(grid_for(f, f->words + 3)), dim3(kThreads), 0,
                     ctx->stream, f->bits.data(), f->words, f->m, f->k, f->length, out);
  OKV_HIP(hipGetLastError());
  if (!dev || !(flags & OKV_F_ASYNC)) OKV_HIP(hipStreamSynchronize(ctx->stream));
  if (!dev) memcpy(dst, f->pin.data(), size_t(need));
  return OKV_OK;
}

uint32_t okv_bloom_last_path(const okv_bloom* f) { return f ? f->last_path : 0; }

}  // extern "C"
