// seek_main.cpp -- okv_seek.hpp on the CPU (tests/test_seek_host.py builds this with
// -fsanitize=address,undefined): the rows RowIter.Seek + Next yield, as the seek kernel
// computes them, against cases written from oracle/pyoracle.py's RowIter.
//
// Case file (little-endian): u32 segments; per segment: u32 rows, per row u32 length and
// the key; u32 blocks, then blocks + 1 u32 first rows; u32 queries, per query u32 length,
// the key, u32 direction, u32 lo, u32 hi.
// Every key and every array of a source are heap copies of their exact size, so a read
// past a key is a sanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "okv_seek.hpp"

namespace {

std::vector<uint8_t> g_file;
size_t g_at = 0;

void need(size_t n) {
  if (g_file.size() - g_at < n) {
    std::fprintf(stderr, "case file truncated at %zu\n", g_at);
    std::exit(2);
  }
}
uint32_t rd32() {
  need(4);
  uint32_t v;
  std::memcpy(&v, g_file.data() + g_at, 4);
  g_at += 4;
  return v;
}
std::string rdkey() {
  const uint32_t n = rd32();
  need(n);
  std::string s(reinterpret_cast<const char*>(g_file.data()) + g_at, n);
  g_at += n;
  return s;
}

std::unique_ptr<uint8_t[]> exact(const void* p, size_t n) {  // (n == 0: a 0-byte block)
  std::unique_ptr<uint8_t[]> q(new uint8_t[n]);
  if (n) std::memcpy(q.get(), p, n);
  return q;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) g_file.insert(g_file.end(), buf, buf + n);
  std::fclose(f);

  const uint32_t nseg = rd32();
  size_t checks = 0;
  int failed = 0;
  for (uint32_t s = 0; s < nseg; ++s) {
    const uint32_t nr = rd32();
    std::vector<uint8_t> arena;
    std::vector<uint64_t> off, first;
    std::vector<uint16_t> len;
    for (uint32_t i = 0; i < nr; ++i) {
      const std::string k = rdkey();
      off.push_back(arena.size());
      len.push_back(uint16_t(k.size()));
      arena.insert(arena.end(), k.begin(), k.end());
    }
    const uint32_t nb = rd32();
    for (uint32_t b = 0; b <= nb; ++b) first.push_back(rd32());
    // the source as the device sees it: exact-size copies
    const auto xa = exact(arena.data(), arena.size());
    const auto xo = exact(off.data(), 8 * size_t(nr)), xl = exact(len.data(), 2 * size_t(nr));
    const auto xf = exact(first.data(), 8 * (size_t(nb) + 1));
    const okv::seek::Source src{xa.get(), reinterpret_cast<const uint64_t*>(xo.get()),
                                reinterpret_cast<const uint16_t*>(xl.get()),
                                reinterpret_cast<const uint64_t*>(xf.get()), nr, nb};
    const uint32_t nq = rd32();
    for (uint32_t q = 0; q < nq; ++q) {
      const std::string ks = rdkey();
      const uint32_t dir = rd32(), want_lo = rd32(), want_hi = rd32();
      const auto k = exact(ks.data(), ks.size());
      uint64_t lo = ~0ull, hi = ~0ull;
      okv::seek::stream(src, k.get(), uint32_t(ks.size()), int(dir), lo, hi);
      if (lo != want_lo || hi != want_hi) {
        std::fprintf(stderr, "FAIL stream: segment %u query %u dir %u: [%llu, %llu) want [%u, %u)\n",
                     s, q, dir, (unsigned long long)lo, (unsigned long long)hi, want_lo, want_hi);
        ++failed;
      }
      ++checks;
    }
  }
  if (g_at != g_file.size()) {
    std::fprintf(stderr, "trailing bytes in the case file\n");
    return 2;
  }
  if (failed) return 1;
  std::printf("all checks passed (%zu)\n", checks);
  return 0;
}
