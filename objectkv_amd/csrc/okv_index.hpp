// okv_index.hpp -- SegmentMetadata.BlockIndex stated once: the order google/btree's
// ReplaceOrInsert gives the index entries (segment_reader.go:234, quirk Q9), the
// lower / upper searches every btree walk of the reader is made of, and the flat image
// of the tree the device floor search reads (okv_get.hip) with that search itself, so
// tests/index_main.cpp runs on the CPU the code the kernel runs.  Internal header; it
// includes no HIP header: floor_upper is __host__ __device__ when a HIP compiler
// defines those, plain inline otherwise.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "okv_sst.h"

#if defined(__host__) && defined(__device__)
#define OKV_INDEX_HD __host__ __device__ inline
#else
#define OKV_INDEX_HD inline
#endif

namespace okv {
namespace index {

// bytes.Compare: -1, 0, 1; a shorter key that is a prefix of the other is smaller.  The
// common bytes go eight at a time as big-endian words (both words hold the same count, so
// they order as the bytes do): on the device the eight loads of a word are independent,
// one memory round trip instead of eight.  No byte past either key is read.
OKV_INDEX_HD int compare(const uint8_t* a, size_t al, const uint8_t* b, size_t bl) {
  const size_t n = al < bl ? al : bl;
  for (size_t i = 0; i < n; i += 8) {
    const size_t m = n - i < 8 ? n - i : 8;
    uint64_t x = 0, y = 0;
#pragma unroll
    for (size_t j = 0; j < 8; ++j) {
      if (j < m) {
        x = (x << 8) | a[i + j];
        y = (y << 8) | b[i + j];
      }
    }
    if (x != y) return x < y ? -1 : 1;
  }
  return al < bl ? -1 : (al > bl ? 1 : 0);
}

// First tree position whose key is >= k (lower) or > k (upper), over nt positions in
// ascending key order; key_of(i, &p, &n) gives the key at position i.  At most 64
// steps (nt < 2^64).  __host__ __device__ like compare: okv_seek.hpp runs them on rows.
template <class KeyOf>
OKV_INDEX_HD size_t lower(size_t nt, KeyOf key_of, const uint8_t* k, size_t kl) {
  size_t lo = 0, hi = nt;
  for (int step = 0; step < 64 && lo < hi; ++step) {
    const size_t m = lo + (hi - lo) / 2;
    const uint8_t* p;
    size_t n;
    key_of(m, &p, &n);
    if (compare(p, n, k, kl) < 0)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}
template <class KeyOf>
OKV_INDEX_HD size_t upper(size_t nt, KeyOf key_of, const uint8_t* k, size_t kl) {
  size_t lo = 0, hi = nt;
  for (int step = 0; step < 64 && lo < hi; ++step) {
    const size_t m = lo + (hi - lo) / 2;
    const uint8_t* p;
    size_t n;
    key_of(m, &p, &n);
    if (compare(p, n, k, kl) <= 0)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}

// The tree after ReplaceOrInsert of entries 0 .. n-1 in meta-block order, as file
// indices in ascending FirstKey order: an entry whose FirstKey equals an earlier one's
// takes its place (Q9), so the last of equal keys stays.  key_of(i, &p, &n): entry i.
template <class KeyOf>
inline std::vector<uint64_t> tree_order(uint64_t n, KeyOf key_of) {
  std::vector<uint64_t> tree;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* k;
    size_t kl;
    key_of(size_t(i), &k, &kl);
    const auto tree_key = [&](size_t t, const uint8_t** p, size_t* pn) {
      key_of(size_t(tree[t]), p, pn);
    };
    const size_t pos = lower(tree.size(), tree_key, k, kl);
    const uint8_t* p = nullptr;
    size_t pn = 0;
    if (pos < tree.size()) tree_key(pos, &p, &pn);
    if (pos < tree.size() && compare(p, pn, k, kl) == 0)
      tree[pos] = i;
    else
      tree.insert(tree.begin() + pos, i);
  }
  return tree;
}

// The first 8 key bytes as a big-endian integer, zero-filled: for keys a and b,
// prefix8(a) < prefix8(b) implies a < b; equal prefixes decide nothing.
OKV_INDEX_HD uint64_t prefix8(const uint8_t* p, size_t n) {
  uint64_t v = 0;
  for (size_t i = 0; i < 8; ++i) v = (v << 8) | (i < n ? p[i] : 0);
  return v;
}

// The tree as flat arrays in tree order (what okv_index_new uploads).
struct Image {
  std::vector<okv_block_desc> descs;
  std::vector<uint32_t> file_index;
  std::vector<uint8_t> arena;  // the first keys, back to back
  std::vector<uint64_t> off;
  std::vector<uint16_t> len;
  std::vector<uint64_t> prefix;
};

// Entries in meta-block order: descs[i], first key fk_arena[fk_off[i] .. +fk_len[i]].
inline Image build_image(const okv_block_desc* descs, const uint8_t* fk_arena,
                         const uint64_t* fk_off, const uint16_t* fk_len, uint64_t n) {
  const auto key_of = [&](size_t i, const uint8_t** p, size_t* pn) {
    *p = fk_arena + fk_off[i];
    *pn = fk_len[i];
  };
  const std::vector<uint64_t> tree = tree_order(n, key_of);
  Image im;
  for (uint64_t e : tree) {
    im.descs.push_back(descs[e]);
    im.file_index.push_back(uint32_t(e));
    im.off.push_back(im.arena.size());
    im.len.push_back(fk_len[e]);
    im.prefix.push_back(prefix8(fk_arena + fk_off[e], fk_len[e]));
    im.arena.insert(im.arena.end(), fk_arena + fk_off[e], fk_arena + fk_off[e] + fk_len[e]);
  }
  return im;
}

// The view of an Image the search reads (host vectors or their device copies).
struct View {
  const uint64_t* prefix;
  const uint8_t* arena;
  const uint64_t* off;
  const uint16_t* len;
  uint64_t nt;
};

inline View view_of(const Image& im) {
  return View{im.prefix.data(), im.arena.data(), im.off.data(), im.len.data(), im.prefix.size()};
}

// a <= b for two keys whose prefix8 tie: the bytes from min(8, shorter length) on (the
// bytes before are equal then) and last the lengths.
OKV_INDEX_HD bool tie_le(const uint8_t* a, uint32_t al, const uint8_t* b, uint32_t bl) {
  const uint32_t n = al < bl ? al : bl;
  int c = 0;
  for (uint32_t j = n < 8 ? n : 8; j < n && c == 0; ++j) c = int(a[j]) - int(b[j]);
  return c != 0 ? c < 0 : al <= bl;
}

// upper(k) over the image: the number of tree entries whose FirstKey <= k, so the
// floor entry of DescendLessOrEqual is the one before it (none when 0).  kp is
// prefix8(k).  A step compares the prefixes; when they tie, tie_le.
// At most 64 steps (nt < 2^64).
OKV_INDEX_HD uint64_t floor_upper(const View& v, const uint8_t* k, uint32_t kl, uint64_t kp) {
  uint64_t lo = 0, hi = v.nt;
  for (int step = 0; step < 64 && lo < hi; ++step) {
    const uint64_t m = lo + (hi - lo) / 2;
    const uint64_t ep = v.prefix[m];
    bool le;  // entry m <= k
    if (ep != kp)
      le = ep < kp;
    else
      le = tie_le(v.arena + v.off[m], v.len[m], k, kl);
    if (le)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}

}  // namespace index
}  // namespace okv
