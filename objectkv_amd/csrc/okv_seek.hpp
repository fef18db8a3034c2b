// okv_seek.hpp -- RowIter(direction).Seek(key) followed by Next() to the end
// (segment_row_iter.go:102-207) stated once, over the decoded rows of a resident
// segment: which rows [lo, hi) the iterator yields.  okv_seek.hip runs it one lane per
// (segment, key, direction) triple and tests/seek_main.cpp runs the same code on the
// CPU.  Internal header; it includes no HIP header (okv_index.hpp's rule): stream is
// __host__ __device__ under a HIP compiler, plain inline otherwise.
//
// Everything is okv_index.hpp's compare / lower / upper over two accessors: the key of
// a row and the FirstKey of a block (the key of the block's first row).  Each search
// takes at most 64 steps and each step compares at most a key length of bytes.
#pragma once
#include <cstddef>
#include <cstdint>

#include "okv_index.hpp"

namespace okv {
namespace seek {

struct Source {  // == okv_seek_src
  const uint8_t* key_arena;
  const uint64_t* key_off;
  const uint16_t* key_len;
  const uint64_t* block_first_row;  // [n_blocks + 1], the last entry is n_rows
  uint64_t n_rows;
  uint64_t n_blocks;
};
static_assert(sizeof(Source) == sizeof(okv_seek_src), "okv_seek_src layout");

constexpr int kAscending = OKV_DIR_ASC, kDescending = OKV_DIR_DESC;

struct RowKey {  // key_of for lower / upper over the rows
  const Source& s;
  OKV_INDEX_HD void operator()(size_t r, const uint8_t** p, size_t* n) const {
    *p = s.key_arena + s.key_off[r];
    *n = s.key_len[r];
  }
};

struct BlockKey {  // ... over the blocks: BlockStat.FirstKey; a block without rows has none
  const Source& s;
  OKV_INDEX_HD void operator()(size_t b, const uint8_t** p, size_t* n) const {
    const uint64_t r = s.block_first_row[b];
    const bool rows = r < s.block_first_row[b + 1];
    *p = rows ? s.key_arena + s.key_off[r] : s.key_arena;
    *n = rows ? s.key_len[r] : 0;
  }
};

// The rows the iterator yields are [lo, hi) in ascending row numbers; a descending
// iterator yields them from hi - 1 down.
//   ascending   Seek parks on the floor block and Next skips rows < key (:170-190): the
//               rows >= key.  UnboundEnd (the key 0xff) parks past the last block (:170).
//   descending  UnboundStart (the empty key) parks below the first block (:203-206).
//               Otherwise DescendLessOrEqual over the block index stops at the last block
//               whose FirstKey <= key, and walks one further when that FirstKey equals
//               the key and a block lies before it (:113-116): the walk then starts at
//               that earlier block's last row, which skips the row equal to the key.
//               From there down Next yields the rows <= key.  A key below every block
//               yields nothing.  UnboundEnd takes every row <= 0xff.
OKV_INDEX_HD void stream(const Source& s, const uint8_t* k, uint32_t kl, int direction,
                         uint64_t& lo, uint64_t& hi) {
  lo = hi = 0;
  if (s.n_blocks == 0 || s.n_rows == 0) return;
  const bool unbound_start = kl == 0, unbound_end = kl == 1 && k[0] == 0xff;
  const RowKey row{s};
  if (direction == kAscending) {
    hi = s.n_rows;
    lo = unbound_end ? s.n_rows : index::lower(size_t(s.n_rows), row, k, kl);
    return;
  }
  if (unbound_start) return;
  uint64_t top = s.n_rows;
  if (!unbound_end) {
    const BlockKey first{s};
    const size_t up = index::upper(size_t(s.n_blocks), first, k, kl);
    if (up == 0) return;
    size_t b = up - 1;
    const uint8_t* fk;
    size_t fl;
    first(b, &fk, &fl);
    if (b > 0 && index::compare(fk, fl, k, kl) == 0) --b;
    top = s.block_first_row[b + 1];
  }
  const uint64_t le = index::upper(size_t(s.n_rows), row, k, kl);
  hi = top < le ? top : le;
}

}  // namespace seek
}  // namespace okv
