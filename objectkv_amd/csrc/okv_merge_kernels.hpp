// okv_merge_kernels.hpp -- the device pieces the k-way merge of one large input set
// (okv_merge.hip, okv_merge_rows) and of many small pages (okv_pages.hip,
// okv_merge_pages) are both made of: the stream descriptor, the key prefix and the byte
// compare, the stream of a global row, and the two statements of the Go loop
// (snapshot_reader.go:214-372) -- a unique key's outcome and the termination key.
// Internal header of those two files; everything is inline device code, so each file's
// code object holds its own kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "okv_ctx.hpp"
#include "okv_kernels.hpp"
#include "okv_sst.h"

namespace okv {
namespace mrg {

struct Src {  // == okv_merge_src
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

constexpr uint32_t kMaxSrc = 64;

// Go loop outcome per unique key
enum : uint8_t {
  kSkip = 0,       // L0 tombstone owner: rolled forward (:316-333)
  kErr = 1,        // ... and a stream ran out on it: Next() returns io.EOF -> error
  kBreak = 2,      // outside the range: break before it (:340-347)
  kEmit = 3,       // appended (:350-354)
  kEmitBreak = 4,  // appended; a stream ran out on it: the stale cursor ends the loop (:336-338)
  kEmitErr = 5,    // appended; the stale cursor's owner is an L0 tombstone: io.EOF error
};

// The first 16 key bytes as two big-endian words, zero padded: with the length
// as the tie-break, comparing these orders keys as bytes.Compare does, so keys
// of <= 16 bytes never touch the arenas.
struct Key16 {
  uint64_t a, b;
};

__device__ __forceinline__ uint32_t find_src(const uint64_t* __restrict__ base, uint32_t k,
                                             uint64_t g) {
  uint32_t lo = 0, hi = k;  // largest i with base[i] <= g
  while (hi - lo > 1) {
    const uint32_t m = (lo + hi) >> 1;
    if (base[m] <= g)
      lo = m;
    else
      hi = m;
  }
  return lo;
}

// Key bytes [off, off + 8) as a big-endian word, bytes past len read as 0;
// the eight loads are independent (one memory round trip).
__device__ __forceinline__ uint64_t be_word(const uint8_t* k, uint32_t len, uint32_t off) {
  uint64_t p = 0;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) p = (p << 8) | (off + i < len ? uint64_t(k[off + i]) : 0ull);
  return p;
}

// The first 16 bytes from the aligned line(s) holding them (the second only
// when the key runs into it: a line holding a valid byte never crosses the
// allocation), bytes past len zeroed, then byte-swapped to big-endian words.
__device__ __forceinline__ Key16 be_prefix(const uint8_t* k, uint32_t len) {
  if (len == 0) return Key16{0, 0};
  const uintptr_t a = reinterpret_cast<uintptr_t>(k);
  const uint4* line = reinterpret_cast<const uint4*>(a & ~uintptr_t(15));
  const uint32_t sh = uint32_t(a & 15), n = len < 16 ? len : 16;
  const uint4 x = line[0];
  const uint4 y = sh + n > 16 ? line[1] : make_uint4(0, 0, 0, 0);
  uint4 v = funnel32(x, y, sh);
  v.x &= byte_mask(0, int32_t(n), 0);
  v.y &= byte_mask(0, int32_t(n), 1);
  v.z &= byte_mask(0, int32_t(n), 2);
  v.w &= byte_mask(0, int32_t(n), 3);
  return Key16{__builtin_bswap64(uint64_t(v.x) | (uint64_t(v.y) << 32)),
               __builtin_bswap64(uint64_t(v.z) | (uint64_t(v.w) << 32))};
}

// bytes.Compare of two keys given their prefixes, lengths and addresses.
__device__ __forceinline__ int key_cmp(const Key16& pa, uint32_t la, const uint8_t* ka,
                                       const Key16& pb, uint32_t lb, const uint8_t* kb) {
  if (pa.a != pb.a) return pa.a < pb.a ? -1 : 1;
  if (pa.b != pb.b) return pa.b < pb.b ? -1 : 1;
  const uint32_t m = la < lb ? la : lb;
  for (uint32_t i = 16; i < m; i += 8) {
    const uint64_t x = be_word(ka, la, i), y = be_word(kb, lb, i);
    if (x != y) return x < y ? -1 : 1;
  }
  return la < lb ? -1 : (la > lb ? 1 : 0);
}

// The Go loop's outcome for one unique key (OKV_MERGE_GETRANGE).  tomb: its owning row
// is an L0 tombstone; end_here: some stream's last row in direction holds this key.
// out_of_range() compares the key with the bound (>= end ascending, <= start
// descending); stale_tomb() says whether the lowest stream that ran out here stands on
// an L0 tombstone.  Both are called only where the Go loop gets that far.
template <class OutOfRange, class StaleTomb>
__device__ __forceinline__ uint8_t go_outcome(bool tomb, bool end_here, OutOfRange out_of_range,
                                              StaleTomb stale_tomb) {
  if (tomb) return end_here ? kErr : kSkip;
  if (out_of_range()) return kBreak;
  if (!end_here) return kEmit;
  return stale_tomb() ? kEmitErr : kEmitBreak;
}

// The termination key of the unique key at direction position d with outcome e, or ~0
// when the loop goes on past it: (position << 3 | code) where code 1 = stop after (OK),
// 2 = stop after with error, 5 = error before, 6 = break before; the limit stops after
// the limit-th emit (emits = emitted keys through d).  A stop after key d and an event
// before key d + 1 share a position; the stop comes first in the Go loop, so its codes
// are the smaller.  The loop ends at the smallest key.
__device__ __forceinline__ unsigned long long term_key(uint8_t e, uint64_t d, uint64_t emits,
                                                       uint64_t limit) {
  if (e == kErr) return (unsigned long long)(d) << 3 | 5;
  if (e == kBreak) return (unsigned long long)(d) << 3 | 6;
  if (e >= kEmit) {
    if (emits == limit || e == kEmitBreak) return (unsigned long long)(d + 1) << 3 | 1;
    if (e == kEmitErr) return (unsigned long long)(d + 1) << 3 | 2;
  }
  return ~0ull;
}

// What a termination key says: the first direction position that is not returned, and
// OKV_M_EOF when the loop ended in io.EOF.
__device__ __host__ inline void term_decode(unsigned long long t, uint64_t nu, uint64_t& stop,
                                            int32_t& status) {
  stop = nu, status = 0;
  if (t == ~0ull) return;
  stop = t >> 3;
  const uint32_t code = uint32_t(t & 7);
  if (code == 2 || code == 5) status = OKV_M_EOF;
}

}  // namespace mrg
}  // namespace okv
