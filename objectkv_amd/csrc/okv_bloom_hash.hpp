// okv_bloom_hash.hpp -- the arithmetic of bloom.BloomFilter.Add / Test, stated once
// for the host and the device (okv_bloom.hip's kernels, tests/bloom_hash_main.cpp).
// Restated from the published algorithms of bits-and-blooms/bloom v2.0.3,
// spaolacci/murmur3 v1.1.0 and willf/bitset v1.1.11 (oracle/bloom_ref.py is the
// independent checker).  Internal header; it includes no HIP header: the functions
// are __host__ __device__ when a HIP compiler defines those, plain inline otherwise.
//
// Key bytes are read as aligned 8-byte words that each contain at least one key
// byte, shifted into place: such a load cannot leave a page the key is mapped on,
// and no other word of the arena is touched (an empty key reads nothing).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__host__) && defined(__device__)
#define OKV_BLOOM_HD __host__ __device__ inline
#else
#define OKV_BLOOM_HD inline
#endif

namespace okv {
namespace bloom {

struct Sum128 {
  uint64_t h1, h2;
};

namespace detail {

typedef uint64_t __attribute__((may_alias)) word_t;

constexpr uint64_t kC1 = 0x87C37B91114253D5ULL, kC2 = 0x4CF5AD432745937FULL;

OKV_BLOOM_HD uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

OKV_BLOOM_HD uint64_t fmix(uint64_t k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDULL;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ULL;
  return k ^ (k >> 33);
}

OKV_BLOOM_HD uint64_t mix_k1(uint64_t k1) { return rotl(k1 * kC1, 31) * kC2; }
OKV_BLOOM_HD uint64_t mix_k2(uint64_t k2) { return rotl(k2 * kC2, 33) * kC1; }

// one 16-byte body block
OKV_BLOOM_HD void body(uint64_t& h1, uint64_t& h2, uint64_t k1, uint64_t k2) {
  h1 ^= mix_k1(k1);
  h1 = rotl(h1, 27) + h2;
  h1 = h1 * 5 + 0x52DCE729;
  h2 ^= mix_k2(k2);
  h2 = rotl(h2, 31) + h1;
  h2 = h2 * 5 + 0x38495AB5;
}

// tail of tl < 16 bytes (t1: bytes 0-7, t2: bytes 8-14, zero beyond tl), then the
// finalisation for a message of n bytes
OKV_BLOOM_HD Sum128 finish(uint64_t h1, uint64_t h2, uint64_t t1, uint64_t t2, unsigned tl,
                           uint64_t n) {
  if (tl > 8) h2 ^= mix_k2(t2);
  if (tl > 0) h1 ^= mix_k1(t1);
  h1 ^= n;
  h2 ^= n;
  h1 += h2;
  h2 += h1;
  h1 = fmix(h1);
  h2 = fmix(h2);
  h1 += h2;
  h2 += h1;
  return Sum128{h1, h2};
}

// The key as little-endian 8-byte pieces, from aligned words.  next() may be
// called while the piece it returns starts inside the key; bytes of the piece
// past the key's end are whatever the last word held (low_bytes() masks them).
struct KeyWords {
  const word_t* q;     // the aligned word holding the next piece's first byte
  const uint8_t* end;  // one past the key
  unsigned sh;         // 8 * (key address mod 8)
  uint64_t cur;        // *q
  OKV_BLOOM_HD KeyWords(const uint8_t* p, size_t n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p) & 7;
    q = reinterpret_cast<const word_t*>(p - a);
    end = p + n;
    sh = unsigned(a) * 8;
    cur = n ? *q : 0;
  }
  OKV_BLOOM_HD uint64_t next() {
    uint64_t piece = cur >> sh;
    ++q;
    const uint64_t nx = reinterpret_cast<const uint8_t*>(q) < end ? *q : 0;
    if (sh) piece |= nx << (64 - sh);
    cur = nx;
    return piece;
  }
};

OKV_BLOOM_HD uint64_t low_bytes(uint64_t x, unsigned nbytes) {  // nbytes in [0, 8]
  return nbytes >= 8 ? x : x & ((uint64_t(1) << (8 * nbytes)) - 1);
}

// state after the floor(n / 16) body blocks, and the tail
struct Walk {
  uint64_t h1, h2, t1, t2;
  unsigned tl;
};

OKV_BLOOM_HD Walk walk(const uint8_t* p, size_t n) {
  Walk w{0, 0, 0, 0, unsigned(n & 15)};
  KeyWords kw(p, n);
  for (size_t b = n / 16; b; --b) {
    const uint64_t k1 = kw.next();
    const uint64_t k2 = kw.next();
    body(w.h1, w.h2, k1, k2);
  }
  if (w.tl > 0) w.t1 = low_bytes(kw.next(), w.tl);
  if (w.tl > 8) w.t2 = low_bytes(kw.next(), w.tl - 8);
  return w;
}

OKV_BLOOM_HD uint64_t mul_hi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return uint64_t((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

}  // namespace detail

// murmur3.Sum128 (MurmurHash3_x64_128, seed 0)
OKV_BLOOM_HD Sum128 murmur3_x64_128(const uint8_t* bytes, size_t n) {
  const detail::Walk w = detail::walk(bytes, n);
  return detail::finish(w.h1, w.h2, w.t1, w.t2, w.tl, n);
}

// bloom.baseHashes: h[0..1] = Sum128(key), h[2..3] = Sum128(key ++ [0x01]).  The
// two messages share every body block of the key, walked once; the 0x01 joins
// the tail, which becomes one more body block when n % 16 == 15.
OKV_BLOOM_HD void base_hashes(const uint8_t* key, size_t n, uint64_t h[4]) {
  const detail::Walk w = detail::walk(key, n);
  const Sum128 a = detail::finish(w.h1, w.h2, w.t1, w.t2, w.tl, n);
  uint64_t h1 = w.h1, h2 = w.h2, t1 = w.t1, t2 = w.t2;
  if (w.tl < 8)
    t1 |= uint64_t(1) << (8 * w.tl);
  else
    t2 |= uint64_t(1) << (8 * (w.tl - 8));
  unsigned tl = w.tl + 1;
  if (tl == 16) {
    detail::body(h1, h2, t1, t2);
    t1 = t2 = 0;
    tl = 0;
  }
  const Sum128 b = detail::finish(h1, h2, t1, t2, tl, uint64_t(n) + 1);
  h[0] = a.h1, h[1] = a.h2, h[2] = b.h1, h[3] = b.h2;
}

// x mod m for a run-time m in [1, 2^64) without a 64-bit division per value:
// r = floor((2^64 - 1) / m), computed once (modulus()).  q = hi64(x * r) is
// floor(x / m) or one less: with 2^64 - 1 = r m + s, 0 <= s < m,
// x / m - x r / 2^64 = x (s + 1) / (m 2^64) < 1.  So x - q m < 2 m (and <= x: no
// wrap), and one conditional subtraction makes it exact.
struct Modulus {
  uint64_t m, r;
};

OKV_BLOOM_HD Modulus modulus(uint64_t m) { return Modulus{m, ~uint64_t(0) / m}; }

OKV_BLOOM_HD uint64_t reduce(uint64_t x, const Modulus& d) {
  const uint64_t rem = x - detail::mul_hi(x, d.r) * d.m;
  return rem >= d.m ? rem - d.m : rem;
}

// bloom.location: (h[i % 2] + i * h[2 + ((i + i % 2) % 4) / 2]) mod m; the sum and
// the product wrap at 2^64 before the reduction, as Go's uint64 does.
OKV_BLOOM_HD uint64_t location(const uint64_t h[4], uint64_t i, const Modulus& m) {
  // blends by mask, not h[i % 2]: an indexed load (which a compiler also makes of a
  // select between two loads) would take h out of registers on the device
  const uint64_t ii = i & 1, jj = ((i + ii) >> 1) & 1;
  const uint64_t a = h[0] ^ ((h[0] ^ h[1]) & (0 - ii));
  const uint64_t b = h[2] ^ ((h[2] ^ h[3]) & (0 - jj));
  return reduce(a + i * b, m);
}

}  // namespace bloom
}  // namespace okv
