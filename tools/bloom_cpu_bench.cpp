// bloom_cpu_bench.cpp -- the host side of tools/bloom_bench.py: BloomFilter.Add over
// every key on T threads, with the arithmetic of okv_bloom_hash.hpp (the statement
// the device kernels use; -O2, no sanitizer).  Threads OR into one filter with
// relaxed atomics.  Build: tools/build_bloom_bench.sh.
//
//   bloom_cpu_bench file  KEYFILE M K THREADS   keys written by bloom_bench.py:
//                                               u64 n, u64 arena bytes, u64 off[n],
//                                               u16 len[n], the arena
//   bloom_cpu_bench fixed N       M K THREADS   key i = i big-endian in 16 bytes
//                                               (okv_synth_rows_fixed)
// Prints one line: rows, threads, seconds, rows/s and the filter's popcount.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "okv_bloom_hash.hpp"

namespace {

struct Filter {
  std::vector<uint64_t> words;
  okv::bloom::Modulus mod;
  uint64_t k;
  void add(const uint8_t* key, size_t n) {
    uint64_t h[4];
    okv::bloom::base_hashes(key, n, h);
    for (uint64_t i = 0; i < k; ++i) {
      const uint64_t loc = okv::bloom::location(h, i, mod);
      __atomic_fetch_or(&words[loc >> 6], uint64_t(1) << (loc & 63), __ATOMIC_RELAXED);
    }
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: bloom_cpu_bench file KEYFILE|fixed N  M K THREADS\n");
    return 2;
  }
  const std::string mode = argv[1];
  const uint64_t m = std::strtoull(argv[3], nullptr, 10), k = std::strtoull(argv[4], nullptr, 10);
  const unsigned threads = unsigned(std::strtoul(argv[5], nullptr, 10));
  if (!m || !threads) return 2;
  Filter f{std::vector<uint64_t>((m + 63) / 64, 0), okv::bloom::modulus(m), k};
  uint64_t n = 0;
  std::vector<uint64_t> off;
  std::vector<uint16_t> len;
  std::vector<uint64_t> arena;  // (8-byte aligned; 8 spare bytes)
  if (mode == "file") {
    std::FILE* fp = std::fopen(argv[2], "rb");
    uint64_t ab = 0;
    if (!fp || std::fread(&n, 8, 1, fp) != 1 || std::fread(&ab, 8, 1, fp) != 1) return 2;
    off.resize(n), len.resize(n), arena.resize(ab / 8 + 2);
    if (std::fread(off.data(), 8, n, fp) != n || std::fread(len.data(), 2, n, fp) != n ||
        std::fread(arena.data(), 1, ab, fp) != ab)
      return 2;
    std::fclose(fp);
  } else {
    n = std::strtoull(argv[2], nullptr, 10);
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < threads; ++t)
    pool.emplace_back([&, t] {
      const uint64_t lo = n * t / threads, hi = n * (t + 1) / threads;
      if (mode == "file") {
        const uint8_t* a = reinterpret_cast<const uint8_t*>(arena.data());
        for (uint64_t i = lo; i < hi; ++i) f.add(a + off[i], len[i]);
      } else {
        alignas(8) uint8_t key[16] = {0};
        for (uint64_t i = lo; i < hi; ++i) {
          for (int b = 0; b < 8; ++b) key[15 - b] = uint8_t(i >> (8 * b));
          f.add(key, 16);
        }
      }
    });
  for (std::thread& t : pool) t.join();
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  uint64_t pop = 0;
  for (uint64_t w : f.words) pop += uint64_t(__builtin_popcountll(w));
  std::printf("cpu_add keys=%s rows=%llu m=%llu k=%llu threads=%u seconds=%.4f rows_per_s=%.4g "
              "popcount=%llu\n", mode.c_str(), (unsigned long long)n, (unsigned long long)m,
              (unsigned long long)k, threads, s, double(n) / s, (unsigned long long)pop);
  return 0;
}
