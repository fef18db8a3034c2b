// index_main.cpp -- okv_index.hpp on the CPU (tests/test_index_host.py builds this with
// -fsanitize=address,undefined): the ReplaceOrInsert order, the lower / upper searches
// and the floor search the device runs over the flat image (floor_upper), against cases
// written from oracle/pyoracle.py's BlockIndex.
//
// Case file (little-endian): u32 trees; per tree: u32 entries, per entry u32 length and
// the first key (meta-block order); u32 tree entries, u32 file index each (tree order);
// u32 queries, per query u32 length, the key, i64 floor file index (-1: none).
// Every key and the image's arena are checked from heap copies of their exact size, so a
// read past a key is a sanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "okv_index.hpp"

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
int64_t rd64() {
  need(8);
  int64_t v;
  std::memcpy(&v, g_file.data() + g_at, 8);
  g_at += 8;
  return v;
}
std::string rdkey() {
  const uint32_t n = rd32();
  need(n);
  std::string s(reinterpret_cast<const char*>(g_file.data()) + g_at, n);
  g_at += n;
  return s;
}

std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t n) {  // (n == 0: a 0-byte block)
  std::unique_ptr<uint8_t[]> q(new uint8_t[n]);
  if (n) std::memcpy(q.get(), p, n);
  return q;
}

int g_failed = 0;
void fail(const char* what, size_t tree, size_t q) {
  std::fprintf(stderr, "FAIL %s: tree %zu query %zu\n", what, tree, q);
  ++g_failed;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) g_file.insert(g_file.end(), buf, buf + n);
  std::fclose(f);

  namespace ix = okv::index;
  const uint32_t ntrees = rd32();
  size_t checks = 0;
  for (uint32_t t = 0; t < ntrees; ++t) {
    const uint32_t ne = rd32();
    std::vector<std::string> keys;
    for (uint32_t i = 0; i < ne; ++i) keys.push_back(rdkey());
    // the C-ABI's layout: descs, arena, off, len in meta-block order
    std::vector<okv_block_desc> descs(ne);
    std::vector<uint8_t> arena;
    std::vector<uint64_t> off;
    std::vector<uint16_t> len;
    for (uint32_t i = 0; i < ne; ++i) {
      descs[i] = okv_block_desc{1000 + i, 0, 0, 0};
      off.push_back(arena.size());
      len.push_back(uint16_t(keys[i].size()));
      arena.insert(arena.end(), keys[i].begin(), keys[i].end());
    }
    const auto arena_x = exact(arena.data(), arena.size());
    const ix::Image im = ix::build_image(descs.data(), arena_x.get(), off.data(), len.data(), ne);

    const uint32_t nt = rd32();
    if (im.file_index.size() != nt) fail("tree size", t, 0);
    const auto key_of = [&](size_t i, const uint8_t** p, size_t* n) {
      *p = arena_x.get() + off[i];
      *n = len[i];
    };
    const std::vector<uint64_t> order = ix::tree_order(ne, key_of);
    for (uint32_t i = 0; i < nt; ++i) {
      const uint32_t want = rd32();
      if (i < im.file_index.size()) {
        if (im.file_index[i] != want || order[i] != want) fail("tree order", t, i);
        if (im.descs[i].offset != 1000 + want) fail("desc order", t, i);
        const std::string& k = keys[want];
        if (im.len[i] != k.size() ||
            std::memcmp(im.arena.data() + im.off[i], k.data(), k.size()) != 0)
          fail("image key", t, i);
        if (im.prefix[i] != ix::prefix8(reinterpret_cast<const uint8_t*>(k.data()), k.size()))
          fail("image prefix", t, i);
        ++checks;
      }
    }
    // the image as the device sees it: exact-size copies
    const auto im_arena = exact(im.arena.data(), im.arena.size());
    const auto im_prefix = exact(reinterpret_cast<const uint8_t*>(im.prefix.data()), 8 * im.prefix.size());
    const auto im_off = exact(reinterpret_cast<const uint8_t*>(im.off.data()), 8 * im.off.size());
    const auto im_len = exact(reinterpret_cast<const uint8_t*>(im.len.data()), 2 * im.len.size());
    const ix::View v{reinterpret_cast<const uint64_t*>(im_prefix.get()), im_arena.get(),
                     reinterpret_cast<const uint64_t*>(im_off.get()),
                     reinterpret_cast<const uint16_t*>(im_len.get()), im.prefix.size()};
    const auto tree_key = [&](size_t i, const uint8_t** p, size_t* n) {
      *p = im_arena.get() + im.off[i];
      *n = im.len[i];
    };

    const uint32_t nq = rd32();
    for (uint32_t q = 0; q < nq; ++q) {
      const std::string ks = rdkey();
      const int64_t want = rd64();
      const auto k = exact(reinterpret_cast<const uint8_t*>(ks.data()), ks.size());
      const size_t up = ix::upper(im.prefix.size(), tree_key, k.get(), ks.size());
      const size_t lo = ix::lower(im.prefix.size(), tree_key, k.get(), ks.size());
      const uint64_t fu = ix::floor_upper(v, k.get(), uint32_t(ks.size()), ix::prefix8(k.get(), ks.size()));
      const int64_t got = up ? int64_t(im.file_index[up - 1]) : -1;
      if (got != want) fail("upper floor", t, q);
      if (fu != up) fail("floor_upper", t, q);
      // lower: the first entry >= k; it differs from upper exactly when k is an entry
      const bool is_entry = up && im.len[up - 1] == ks.size() &&
                            std::memcmp(im_arena.get() + im.off[up - 1], k.get(), ks.size()) == 0;
      if (lo != (is_entry ? up - 1 : up)) fail("lower", t, q);
      checks += 3;
    }
  }
  if (g_at != g_file.size()) {
    std::fprintf(stderr, "trailing bytes in the case file\n");
    return 2;
  }
  if (g_failed) return 1;
  std::printf("all checks passed (%zu)\n", checks);
  return 0;
}
