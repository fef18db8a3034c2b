// okv_snap_route.hpp -- snapshot_reader.Reader.getPossibleSegmentsForKey
// (snapshot_reader.go:152-171) stated once: the flat image of blockRangeTree the
// device reads (okv_snap.hip) and the walk itself, so tests/snap_route_main.cpp runs on
// the CPU the code the route kernel runs.  Internal header; it includes no HIP header
// (okv_index.hpp's rule): candidates is __host__ __device__ under a HIP compiler, plain
// inline otherwise.
//
// The records come in tree order -- blockRangeLessFunc (:28-60): FirstKey, then an
// empty LastKey last, LastKey, then ID -- which the host computes; FirstKey ascending is
// all the walk relies on.  DescendLessOrEqual from the pivot {FirstKey: key} starts at
// the last record whose FirstKey <= key (the pivot's empty LastKey makes it the greatest
// of its FirstKey) and getPossibleSegmentsForKey collects records while
// FirstKey <= key <= LastKey, stopping at the first that fails: a record below a
// non-covering one is never reached, even when it holds the key.
#pragma once
#include <cstdint>
#include <vector>

#include "okv_index.hpp"

namespace okv {
namespace snap_route {

// blockRangeTree as flat arrays in tree order (what okv_snap_new uploads): first and
// last keys in one arena, each with off / len and its 8-byte big-endian prefix.
struct Image {
  std::vector<uint8_t> arena;
  std::vector<uint64_t> first_off, last_off;
  std::vector<uint16_t> first_len, last_len;
  std::vector<uint64_t> first_prefix, last_prefix;
  std::vector<uint32_t> level, priority;
};

inline void add_record(Image& im, const uint8_t* first, uint16_t fl, const uint8_t* last,
                       uint16_t ll, uint32_t level, uint32_t priority) {
  im.first_off.push_back(im.arena.size());
  im.first_len.push_back(fl);
  im.first_prefix.push_back(index::prefix8(first, fl));
  im.arena.insert(im.arena.end(), first, first + fl);
  im.last_off.push_back(im.arena.size());
  im.last_len.push_back(ll);
  im.last_prefix.push_back(index::prefix8(last, ll));
  im.arena.insert(im.arena.end(), last, last + ll);
  im.level.push_back(level);
  im.priority.push_back(priority);
}

// The view the walk reads (host vectors or their device copies).
struct View {
  index::View first;  // the FirstKeys as okv_index.hpp's search reads them
  const uint64_t* last_prefix;
  const uint64_t* last_off;
  const uint16_t* last_len;
};

inline View view_of(const Image& im) {
  return View{index::View{im.first_prefix.data(), im.arena.data(), im.first_off.data(),
                          im.first_len.data(), im.first_prefix.size()},
              im.last_prefix.data(), im.last_off.data(), im.last_len.data()};
}

// key <= record t's LastKey, by okv_index.hpp's compare: prefix, then tie_le
OKV_INDEX_HD bool covers(const View& v, uint64_t t, const uint8_t* k, uint32_t kl, uint64_t kp) {
  const uint64_t lp = v.last_prefix[t];
  if (lp != kp) return kp < lp;
  return index::tie_le(k, kl, v.first.arena + v.last_off[t], v.last_len[t]);
}

// The tree positions the Go walk collects for k are [lo, hi), visited from hi - 1 down;
// kp is prefix8(k).  At most 64 search steps and hi - lo <= nt walk steps.
OKV_INDEX_HD void candidates(const View& v, const uint8_t* k, uint32_t kl, uint64_t kp,
                             uint64_t& lo, uint64_t& hi) {
  hi = index::floor_upper(v.first, k, kl, kp);
  lo = hi;
  while (lo > 0 && covers(v, lo - 1, k, kl, kp)) --lo;
}

}  // namespace snap_route
}  // namespace okv
