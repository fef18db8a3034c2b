// okv_stage.hpp -- host mode of the batched calls stated once: the key check of an
// okv_rows, the 256-byte-aligned layout of a staging buffer, and the copies of the key
// arrays and the per-key columns in and out of it (okv_bloom.hip, okv_get.hip,
// okv_snap.hip, okv_seek.hip).  Internal header.  DESIGN.md 13.7.6.
//
// The first part is plain C++ and includes no HIP header (tests/stage_main.cpp runs it on
// the CPU); the second needs okv_ctx.hpp included first, which defines OKV_BUF_HIP.
#pragma once
#include <cstddef>
#include <cstdint>

#include "okv_sst.h"

namespace okv {
namespace stage {

// Offsets into one staging buffer: every region starts on a 256-byte line.
class Layout {
 public:
  size_t add(size_t bytes) {
    const size_t at = end();
    end_ = at + bytes;
    return at;
  }
  size_t end() const { return (end_ + 255) & ~size_t(255); }  // the room to reserve

 private:
  size_t end_ = 0;
};

// The key arrays of `rows`: each present (the arena may be NULL when it has no bytes)
// and, with `bounds` (host arrays only), every key inside key_arena_bytes.  No rows need
// no arrays: the entry points return before they look.
enum class Keys { ok, null_array, outside };
inline Keys check_keys(const okv_rows* rows, bool bounds) {
  if (rows->n_rows == 0) return Keys::ok;
  if (!rows->key_off || !rows->key_len || (!rows->key_arena && rows->key_arena_bytes))
    return Keys::null_array;
  for (uint64_t i = 0; bounds && i < rows->n_rows; ++i)  // (no off + len: it could wrap)
    if (rows->key_off[i] > rows->key_arena_bytes ||
        rows->key_len[i] > rows->key_arena_bytes - rows->key_off[i])
      return Keys::outside;
  return Keys::ok;
}

// One per-element array of a call.  `in`: copied to the device before the kernels;
// `out`: copied back after them, unless the caller left `host` NULL (an optional output
// the kernels write all the same).  dev is where the kernels find it: base + off of the
// staging buffer, or `host` itself when the caller's arrays are device memory.
struct Col {
  const void* host;
  size_t elem;  // bytes per element
  bool in, out;
  void* dev = nullptr;
  size_t off = 0;
  template <class T>
  T* as() const { return static_cast<T*>(dev); }
};

inline void place(Layout& L, Col* cols, size_t ncols, size_t n) {
  for (size_t c = 0; c < ncols; ++c) cols[c].off = L.add(cols[c].elem * n);
}
inline void bind(uint8_t* base, Col* cols, size_t ncols) {
  for (size_t c = 0; c < ncols; ++c) cols[c].dev = base + cols[c].off;
}
inline void direct(Col* cols, size_t ncols) {  // device mode: the caller's arrays
  for (size_t c = 0; c < ncols; ++c) cols[c].dev = const_cast<void*>(cols[c].host);
}

}  // namespace stage

#ifdef OKV_BUF_HIP
namespace {  // (internal linkage, as the kernels that take a KeyRows)

struct KeyRows {  // the key arrays as the kernels read them
  const uint8_t* ka;
  const uint64_t* ko;
  const uint16_t* kl;
  uint64_t n;
};

// OKV_E_ARG with the caller's prefix ("get", "snap get", ...) when the check failed.
inline int key_err(okv_ctx* ctx, stage::Keys k, const char* prefix, const char* null_what) {
  if (k == stage::Keys::ok) return OKV_OK;
  const std::string what = std::string(prefix) + ": " +
      (k == stage::Keys::null_array ? null_what : "a key lies outside key_arena_bytes");
  return set_err(ctx, OKV_E_ARG, what.c_str());
}

// The columns bound to the staging buffer at `base`, the `in` ones copied to it: one
// hipMemcpyAsync each, from the caller's memory.
inline int stage_in(okv_ctx* ctx, uint8_t* base, stage::Col* cols, size_t ncols, size_t n) {
  stage::bind(base, cols, ncols);
  for (size_t c = 0; c < ncols; ++c)
    if (cols[c].in)
      OKV_HIP(hipMemcpyAsync(cols[c].dev, cols[c].host, cols[c].elem * n, hipMemcpyHostToDevice,
                             ctx->stream));
  return OKV_OK;
}

// The `out` columns the caller gave copied back: one hipMemcpyAsync each, not awaited.
inline int stage_out(okv_ctx* ctx, const stage::Col* cols, size_t ncols, size_t n) {
  for (size_t c = 0; c < ncols; ++c)
    if (cols[c].out && cols[c].host)
      OKV_HIP(hipMemcpyAsync(const_cast<void*>(cols[c].host), cols[c].dev, cols[c].elem * n,
                             hipMemcpyDeviceToHost, ctx->stream));
  return OKV_OK;
}

// The key arrays of `rows` (checked; null_what names them in the message) and the
// columns as device pointers.  Device mode: the caller's.  Host mode: `buf` laid out as
// arena, offsets, lengths, then the columns; the three key arrays and the `in` columns
// copied in, in that order.
inline int stage_keys(okv_ctx* ctx, DevBuf<uint8_t>& buf, const okv_rows* rows, bool dev,
                      const char* prefix, const char* null_what, stage::Col* cols,
                      size_t ncols, KeyRows* R) {
  if (int rc = key_err(ctx, stage::check_keys(rows, !dev), prefix, null_what)) return rc;
  const uint64_t n = R->n = rows->n_rows;
  if (dev) {
    R->ka = rows->key_arena, R->ko = rows->key_off, R->kl = rows->key_len;
    stage::direct(cols, ncols);
    return OKV_OK;
  }
  stage::Col k[3] = {{rows->key_arena, 1, rows->key_arena_bytes != 0, false},
                     {rows->key_off, 8, true, false},
                     {rows->key_len, 2, true, false}};
  stage::Layout L;
  stage::place(L, k, 1, rows->key_arena_bytes);
  stage::place(L, k + 1, 2, n);
  stage::place(L, cols, ncols, n);
  if (int rc = reserve(ctx, buf, L.end())) return rc;
  if (int rc = stage_in(ctx, buf.data(), k, 1, rows->key_arena_bytes)) return rc;
  if (int rc = stage_in(ctx, buf.data(), k + 1, 2, n)) return rc;
  R->ka = k[0].as<const uint8_t>(), R->ko = k[1].as<const uint64_t>();
  R->kl = k[2].as<const uint16_t>();
  return stage_in(ctx, buf.data(), cols, ncols, n);
}

}  // namespace
#endif

}  // namespace okv
