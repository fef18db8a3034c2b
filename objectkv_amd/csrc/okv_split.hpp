// okv_split.hpp -- the range-split rule of okv_encode_split, stated once for the host and
// the device (okv_split.inc's kernels, tests/split_main.cpp).  Internal header; it includes
// no HIP header: the functions are __host__ __device__ when a HIP compiler defines those,
// plain inline otherwise.
//
// The rows are cut into blocks by the encoder's greedy chain.  A segment is a run of
// consecutive blocks of that chain: the segment starting at block i ends with the first
// block j >= i for which sum BlockSize[i..j] >= split_bytes (split_bytes != 0) or
// rows(i..j) >= split_rows (split_rows != 0); if neither holds before the last block it ends
// with the last block (sst/COMPACTION.md "Ranges should be split by size at compaction
// time"; a Go caller watching the writer's flushed bytes and rows and closing after a flush).
//
// Both sums are differences of exclusive prefixes over the blocks, P(0) = 0 .. P(nb) = the
// total, strictly increasing (a block has at least DataBlockSize bytes and one row), given as
// callables so the device reads the plan's arrays and the test plain vectors.
#pragma once
#include <cstdint>

#if defined(__host__) && defined(__device__)
#define OKV_SPLIT_HD __host__ __device__ inline
#else
#define OKV_SPLIT_HD inline
#endif

namespace okv {
namespace split {

// min(end, the smallest e in (i, end] with P(e) - P(i) >= t), for i < end: a binary search of
// at most 64 probes.
template <class Pre>
OKV_SPLIT_HD uint64_t reach(uint64_t i, uint64_t end, uint64_t t, Pre P) {
  const uint64_t base = P(i);
  uint64_t lo = i + 1, hi = end;  // the answer lies in [lo, hi]
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (P(mid) - base >= t)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// The first block of the segment after the one that starts at block i < nb (nb: there is
// none).  B, R: the exclusive prefixes of BlockSize and of rows over the blocks.
template <class PreB, class PreR>
OKV_SPLIT_HD uint64_t next(uint64_t i, uint64_t nb, uint64_t split_bytes, uint64_t split_rows,
                           PreB B, PreR R) {
  uint64_t e = nb;
  if (split_bytes) e = reach(i, e, split_bytes, B);
  if (split_rows) e = reach(i, e, split_rows, R);  // (within the byte bound: the earlier wins)
  return e;
}

// The chain 0, next(0), next(next(0)), .. nb by pointer jumping over nb + 1 nodes, node nb a
// fixed point.  Round k holds J_k = next^(2^k); every marked node i marks J_k[i], and
// J_(k+1)[i] = J_k[J_k[i]].  With mark[0] set before round 0, after round k the marked nodes
// are the chain's first 2^(k+1) (every node a round marks is on the chain, so a mark that
// lands during the round it is read in only marks more of the chain early).  rounds(nb)
// rounds mark the whole chain.
OKV_SPLIT_HD uint32_t rounds(uint64_t nb) {
  uint32_t r = 0;
  while (r < 64 && (uint64_t(1) << r) < nb + 1) ++r;
  return r;
}

// One node's step of a round: returns J_(k+1)[i]; *mark_target = J_k[i], the node to mark
// when i is marked.
OKV_SPLIT_HD uint32_t jump(const uint32_t* jk, uint64_t i, uint32_t* mark_target) {
  const uint32_t j = jk[i];
  *mark_target = j;
  return jk[j];
}

OKV_SPLIT_HD uint64_t round16(uint64_t x) { return (x + 15) & ~uint64_t(15); }

// generateMetaBlock's bytes before the block index: u16 + FirstKey, u16 + LastKey, the bloom
// flag [+ u64 length + the filter's WriteTo bytes], the compression byte, the index-type
// byte, the u64 entry count.  bloom_bytes: 0 for a nil filter.
OKV_SPLIT_HD uint64_t meta_head(uint64_t first_key_len, uint64_t last_key_len,
                                uint64_t bloom_bytes) {
  return 2 + first_key_len + 2 + last_key_len + 1 + (bloom_bytes ? 8 + bloom_bytes : 0) + 1 + 1 +
         8;
}

}  // namespace split
}  // namespace okv
