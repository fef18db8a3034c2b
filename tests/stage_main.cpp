// stage_main.cpp -- the plain C++ part of okv_stage.hpp on the CPU (tests/test_stage_host.py
// builds this with -fsanitize=address,undefined): Layout, place and check_keys, one answer
// line per case line of the file named by argv[1].  What the answers must be is stated in
// the Python test, not here.
//
//   layout SET n key_arena_bytes nsrc
//       the staging layout of a call, as its entry point places it
//       -> "layout" then offset:bytes of every region in placement order, then end()
//   keys bounds arena_null off_null len_null key_arena_bytes n off0 len0 off1 len1 ...
//       check_keys over heap copies of the exact size (an over-read is a sanitizer error)
//       -> "keys ok" | "keys null_array" | "keys outside"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "okv_stage.hpp"

using okv::stage::Col;
using okv::stage::Layout;

namespace {

constexpr size_t kSeekSource = sizeof(okv_seek_src);  // (== seek::Source, okv_seek.hpp)

Col col(size_t elem) { return Col{nullptr, elem, false, true}; }

// The regions of each call in the order its entry point places them: (Col, elements).
std::vector<std::pair<Col, size_t>> regions(const std::string& set, size_t n, size_t kab,
                                            size_t nsrc) {
  std::vector<std::pair<Col, size_t>> r;
  const auto keys = [&] { r = {{col(1), kab}, {col(8), n}, {col(2), n}}; };
  const auto per_key = [&](std::initializer_list<size_t> elems) {
    for (size_t e : elems) r.push_back({col(e), n});
  };
  if (set == "bloom_add") keys();
  if (set == "bloom_test") keys(), per_key({1});
  if (set == "get") keys(), per_key({4, 4, 4, 8, 4, 8});
  if (set == "snap") keys(), per_key({4, 4, 4, 4, 8, 4, 8});
  if (set == "gather") per_key({8, 2, 8, 4});
  if (set == "seek") {
    r = {{col(kab), 1}, {col(kSeekSource * nsrc), 1}};
    per_key({8, 2, 4, 1, 16});
  }
  return r;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string what;
    ss >> what;
    if (what == "layout") {
      std::string set;
      size_t n, kab, nsrc;
      ss >> set >> n >> kab >> nsrc;
      auto r = regions(set, n, kab, nsrc);
      if (r.empty()) return 3;
      Layout L;
      for (auto& [c, count] : r) okv::stage::place(L, &c, 1, count);
      std::cout << "layout";
      for (auto& [c, count] : r) std::cout << ' ' << c.off << ':' << c.elem * count;
      std::cout << ' ' << L.end() << '\n';
    } else if (what == "keys") {
      int bounds, arena_null, off_null, len_null;
      uint64_t kab, n;
      ss >> bounds >> arena_null >> off_null >> len_null >> kab >> n;
      std::unique_ptr<uint64_t[]> off(new uint64_t[n]);
      std::unique_ptr<uint16_t[]> len(new uint16_t[n]);
      for (uint64_t i = 0; i < n; ++i) {
        uint64_t l;
        ss >> off[i] >> l;
        len[i] = uint16_t(l);
      }
      if (!ss) return 4;
      const uint8_t arena = 0;  // (check_keys never reads the arena)
      okv_rows rows;
      std::memset(&rows, 0, sizeof(rows));
      rows.key_arena = arena_null ? nullptr : &arena;
      rows.key_off = off_null ? nullptr : off.get();
      rows.key_len = len_null ? nullptr : len.get();
      rows.n_rows = n, rows.key_arena_bytes = kab;
      const okv::stage::Keys k = okv::stage::check_keys(&rows, bounds != 0);
      std::cout << "keys "
                << (k == okv::stage::Keys::ok ? "ok"
                    : k == okv::stage::Keys::null_array ? "null_array" : "outside")
                << '\n';
    } else {
      return 5;
    }
  }
  std::cout << "done\n";
  return 0;
}
