// bloom_hash_main.cpp -- okv_bloom_hash.hpp on the CPU, against a case file that
// tests/test_bloom_host.py writes from oracle/bloom_ref.py.  Host only; built with
// AddressSanitizer and UBSan, links no HIP, never loaded into Python.
//
// Case file (little endian): u32 nkeys, then per key u32 len, the bytes, u64 h[4];
// u32 nm, u64 m[nm]; u32 nk, u64 k[nk]; then for key, for m, for k: k u64 locations.
//
// Every key is hashed at byte offsets 0..7 of a buffer in which only the aligned
// 8-byte words that contain a key byte are addressable (the rest is poisoned
// under AddressSanitizer): a load of any other word aborts the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "okv_bloom_hash.hpp"

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define BLOOM_POISON(p, n) __asan_poison_memory_region((p), (n))
#define BLOOM_UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#endif
#ifndef BLOOM_POISON
#define BLOOM_POISON(p, n) ((void)(p), (void)(n))
#define BLOOM_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

namespace {

int failures = 0;

void fail(const char* what, size_t key, size_t a, size_t b) {
  if (++failures <= 20) std::fprintf(stderr, "FAIL %s: key %zu (%zu, %zu)\n", what, key, a, b);
}

struct Reader {
  std::vector<uint8_t> d;
  size_t at = 0;
  const uint8_t* take(size_t n) {
    if (at + n > d.size()) {
      std::fprintf(stderr, "case file too short\n");
      std::exit(2);
    }
    at += n;
    return d.data() + at - n;
  }
  uint32_t u32() {
    uint32_t v;
    std::memcpy(&v, take(4), 4);
    return v;
  }
  uint64_t u64() {
    uint64_t v;
    std::memcpy(&v, take(8), 8);
    return v;
  }
};

struct Key {
  std::vector<uint8_t> bytes;
  uint64_t h[4];
};

constexpr size_t kGuard = 64;

// the key at offset `off` of a buffer whose other words are poisoned
struct Placed {
  uint8_t* buf;
  size_t cap;
  const uint8_t* key;
  Placed(const std::vector<uint8_t>& bytes, size_t off) {
    cap = kGuard + ((bytes.size() + 8 + 7) & ~size_t(7)) + kGuard;
    buf = static_cast<uint8_t*>(std::aligned_alloc(64, (cap + 63) & ~size_t(63)));
    if (!buf) std::exit(2);
    std::memset(buf, 0xA5, cap);
    uint8_t* p = buf + kGuard + off;
    if (!bytes.empty()) std::memcpy(p, bytes.data(), bytes.size());
    key = p;
    BLOOM_POISON(buf, cap);
    if (!bytes.empty()) {
      const uintptr_t lo = reinterpret_cast<uintptr_t>(p) & ~uintptr_t(7);
      const uintptr_t hi = (reinterpret_cast<uintptr_t>(p) + bytes.size() + 7) & ~uintptr_t(7);
      BLOOM_UNPOISON(reinterpret_cast<void*>(lo), hi - lo);
    }
  }
  ~Placed() {
    BLOOM_UNPOISON(buf, cap);
    std::free(buf);
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: bloom_hash_main CASEFILE\n");
    return 2;
  }
  Reader r;
  {
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint8_t chunk[65536];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof chunk, f)) > 0) r.d.insert(r.d.end(), chunk, chunk + n);
    std::fclose(f);
  }
  std::vector<Key> keys(r.u32());
  for (Key& k : keys) {
    const uint32_t len = r.u32();
    const uint8_t* b = r.take(len);
    k.bytes.assign(b, b + len);
    for (uint64_t& h : k.h) h = r.u64();
  }
  std::vector<uint64_t> ms(r.u32());
  for (uint64_t& m : ms) m = r.u64();
  std::vector<uint64_t> ks(r.u32());
  for (uint64_t& k : ks) k = r.u64();

  size_t checked = 0;
  for (size_t ki = 0; ki < keys.size(); ++ki) {
    const Key& k = keys[ki];
    std::vector<uint8_t> plus = k.bytes;  // key ++ [0x01]
    plus.push_back(1);
    for (size_t off = 0; off < 8; ++off) {
      uint64_t h[4];
      {
        Placed pk(k.bytes, off);
        okv::bloom::base_hashes(pk.key, k.bytes.size(), h);
        for (int j = 0; j < 4; ++j)
          if (h[j] != k.h[j]) fail("base_hashes", ki, off, size_t(j));
        const okv::bloom::Sum128 s = okv::bloom::murmur3_x64_128(pk.key, k.bytes.size());
        if (s.h1 != k.h[0] || s.h2 != k.h[1]) fail("murmur3_x64_128(key)", ki, off, 0);
      }
      Placed pp(plus, off);
      const okv::bloom::Sum128 s = okv::bloom::murmur3_x64_128(pp.key, plus.size());
      if (s.h1 != k.h[2] || s.h2 != k.h[3]) fail("murmur3_x64_128(key ++ 1)", ki, off, 0);
      checked += 3;
    }
    for (size_t mi = 0; mi < ms.size(); ++mi) {
      const okv::bloom::Modulus d = okv::bloom::modulus(ms[mi]);
      for (size_t kj = 0; kj < ks.size(); ++kj)
        for (uint64_t i = 0; i < ks[kj]; ++i) {
          const uint64_t want = r.u64();
          if (okv::bloom::location(k.h, i, d) != want) fail("location", ki, mi, size_t(i));
          ++checked;
        }
    }
  }
  if (r.at != r.d.size()) {
    std::fprintf(stderr, "case file has %zu unread bytes\n", r.d.size() - r.at);
    return 1;
  }
  // the reduction alone at the ends of its range
  const uint64_t edge[] = {0, 1, 2, 63, 64, (uint64_t(1) << 32) - 1, uint64_t(1) << 32,
                           (uint64_t(1) << 63) - 1, uint64_t(1) << 63, ~uint64_t(0) - 1, ~uint64_t(0)};
  for (uint64_t m : ms)
    for (uint64_t x : edge) {
      if (okv::bloom::reduce(x, okv::bloom::modulus(m)) != x % m) fail("reduce", 0, size_t(m), size_t(x));
      ++checked;
    }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("%zu values: all checks passed\n", checked);
  return 0;
}
