// snap_route_main.cpp -- okv_snap_route.hpp on the CPU (tests/test_snap_route_host.py
// builds this with -fsanitize=address,undefined): the flat image of blockRangeTree and
// the walk of getPossibleSegmentsForKey the route kernel runs (candidates), against
// cases written from oracle/snapshot_oracle.py's Reader.
//
// Case file (little-endian): u32 snapshots; per snapshot: u32 records, per record (tree
// order) u32 length and the first key, u32 length and the last key, u32 level, u32
// priority; u32 queries, per query u32 length, the key, u32 lo, u32 hi (the walk
// collects tree positions hi - 1 down to lo).
// Every key and every array of the image are checked from heap copies of their exact
// size, so a read past a key is a sanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "okv_snap_route.hpp"

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
const uint8_t* bytes(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) g_file.insert(g_file.end(), buf, buf + n);
  std::fclose(f);

  namespace sr = okv::snap_route;
  const uint32_t nsnap = rd32();
  size_t checks = 0;
  int failed = 0;
  for (uint32_t s = 0; s < nsnap; ++s) {
    const uint32_t nr = rd32();
    sr::Image im;
    for (uint32_t i = 0; i < nr; ++i) {
      const std::string first = rdkey(), last = rdkey();
      const uint32_t level = rd32(), priority = rd32();
      const auto fx = exact(first.data(), first.size()), lx = exact(last.data(), last.size());
      sr::add_record(im, fx.get(), uint16_t(first.size()), lx.get(), uint16_t(last.size()), level,
                     priority);
      if (im.level.back() != level || im.priority.back() != priority ||
          im.first_prefix.back() != okv::index::prefix8(bytes(first), first.size()) ||
          im.last_prefix.back() != okv::index::prefix8(bytes(last), last.size())) {
        std::fprintf(stderr, "FAIL image: snapshot %u record %u\n", s, i);
        ++failed;
      }
    }
    // the image as the device sees it: exact-size copies
    const auto arena = exact(im.arena.data(), im.arena.size());
    const auto fp = exact(im.first_prefix.data(), 8 * size_t(nr)), fo = exact(im.first_off.data(), 8 * size_t(nr));
    const auto fl = exact(im.first_len.data(), 2 * size_t(nr));
    const auto lp = exact(im.last_prefix.data(), 8 * size_t(nr)), lo_ = exact(im.last_off.data(), 8 * size_t(nr));
    const auto ll = exact(im.last_len.data(), 2 * size_t(nr));
    const sr::View v{okv::index::View{reinterpret_cast<const uint64_t*>(fp.get()), arena.get(),
                                      reinterpret_cast<const uint64_t*>(fo.get()),
                                      reinterpret_cast<const uint16_t*>(fl.get()), nr},
                     reinterpret_cast<const uint64_t*>(lp.get()),
                     reinterpret_cast<const uint64_t*>(lo_.get()),
                     reinterpret_cast<const uint16_t*>(ll.get())};
    const uint32_t nq = rd32();
    for (uint32_t q = 0; q < nq; ++q) {
      const std::string ks = rdkey();
      const uint32_t want_lo = rd32(), want_hi = rd32();
      const auto k = exact(ks.data(), ks.size());
      uint64_t lo = ~0ull, hi = ~0ull;
      sr::candidates(v, k.get(), uint32_t(ks.size()), okv::index::prefix8(k.get(), ks.size()), lo, hi);
      if (lo != want_lo || hi != want_hi) {
        std::fprintf(stderr, "FAIL candidates: snapshot %u query %u: [%llu, %llu) want [%u, %u)\n", s,
                     q, (unsigned long long)lo, (unsigned long long)hi, want_lo, want_hi);
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
