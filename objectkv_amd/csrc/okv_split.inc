// okv_split.inc -- okv_encode_split: a compaction's output segments from one call.  Included
// at the end of okv_encode.hip, whose plan (enc_plan), pack launch (enc_pack) and scratch
// (EncScratch) it uses unchanged; the rule itself is okv_split.hpp.  DESIGN.md 28.
//
// After the plan and the pack (the data arena is okv_encode_rows' data blocks):
//   S1 okv_split_next_kernel     next(i) per block (two bounded binary searches), mark[0]
//   S2 okv_split_jump_kernel     one pointer-jumping round, rounds(nb) launches
//   S3 okv_split_number_kernel   tile-local scan of the marks (+ okv_enc_scan_kernel over tiles)
//   S4 okv_split_start_kernel    first block of every segment
//   S5 okv_split_layout_kernel   per segment: rows, data span, meta head and length
//                                (+ okv_enc_scan_kernel of round16(meta_bytes + 25) -> meta_off)
//   S6 okv_split_meta_kernel     one lane per block: its BlockStat entry (Offset relative to
//                                its segment); the lane of a segment's first block also writes
//                                the segment's meta head
//   S7 okv_split_bloom_add_kernel / S8 okv_split_bloom_write_kernel   per-segment filters
//   S9 okv_hash_kernel over one descriptor per meta block
//   S10 okv_split_trailer_kernel one lane per segment: meta_hash and the 25-byte trailer
// No workgroup waits for another, no memory is spun on, and every loop is bounded by an
// argument of the call (DESIGN.md 25.2).
#include "okv_bloom_hash.hpp"
#include "okv_split.hpp"

namespace okv {

// exclusive prefixes over the blocks, from the plan's arrays
struct SplitBytePre {
  const Desc* desc;
  uint64_t nb, total;
  __device__ uint64_t operator()(uint64_t k) const { return k < nb ? desc[k].offset : total; }
};
struct SplitRowPre {
  const uint64_t* first;  // [nb + 1]
  __device__ uint64_t operator()(uint64_t k) const { return first[k]; }
};
struct SplitEntPre {  // meta index entry bytes before block k
  const uint64_t* moff;
  uint64_t nb, head, total;
  __device__ uint64_t operator()(uint64_t k) const { return k < nb ? moff[k] - head : total; }
};

__global__ __launch_bounds__(kThreads) void okv_split_next_kernel(
    const Desc* __restrict__ desc, const uint64_t* __restrict__ first, uint64_t nb,
    uint64_t data_bytes, uint64_t split_bytes, uint64_t split_rows, uint32_t* __restrict__ j0,
    uint32_t* __restrict__ mark) {
  const uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i > nb) return;
  j0[i] = i < nb ? uint32_t(split::next(i, nb, split_bytes, split_rows,
                                        SplitBytePre{desc, nb, data_bytes}, SplitRowPre{first}))
                 : uint32_t(nb);
  mark[i] = i == 0;
}

__global__ __launch_bounds__(kThreads) void okv_split_jump_kernel(
    const uint32_t* __restrict__ jk, uint32_t* __restrict__ jn, uint32_t* mark, uint64_t nb) {
  const uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i > nb) return;
  uint32_t t;
  jn[i] = split::jump(jk, i, &t);
  // (a mark another lane sets during this round names a chain node too: okv_split.hpp)
  if (__atomic_load_n(&mark[i], __ATOMIC_RELAXED)) __atomic_store_n(&mark[t], 1u, __ATOMIC_RELAXED);
}

__global__ __launch_bounds__(kThreads) void okv_split_number_kernel(
    const uint32_t* __restrict__ mark, uint64_t nb, uint32_t* __restrict__ xl,
    uint64_t* __restrict__ tile_tot) {
  __shared__ uint64_t sm[kThreads / 64 + 1];
  const uint64_t base = uint64_t(blockIdx.x) * kETile + uint64_t(threadIdx.x) * kEItems;
  uint32_t m[kEItems];
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < kEItems; ++i) {
    m[i] = base + i < nb ? mark[base + i] : 0;
    s += m[i];
  }
  uint64_t tot;
  uint64_t x = wg_excl_scan(s, sm, tot);
#pragma unroll
  for (int i = 0; i < kEItems; ++i) {
    if (base + i < nb) xl[base + i] = uint32_t(x);
    x += m[i];
  }
  if (threadIdx.x == 0) tile_tot[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kThreads) void okv_split_start_kernel(
    const uint32_t* __restrict__ mark, const uint32_t* __restrict__ xl,
    const uint64_t* __restrict__ tile_pre, uint64_t nb, const unsigned long long* __restrict__ tot,
    uint32_t* __restrict__ fb) {
  const uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= nb) return;
  if (i == 0) fb[min(tot[0], (unsigned long long)nb)] = uint32_t(nb);
  if (mark[i]) fb[tile_pre[i / kETile] + xl[i]] = uint32_t(i);
}

struct SplitLayoutParams {
  const uint32_t* fb;
  uint64_t S, nb;
  const Desc* desc;
  const uint64_t* first;
  const uint64_t* moff;
  const uint16_t* key_len;
  uint64_t data_bytes, meta_ent, head_whole, bloom_bytes;
  okv_split_seg* segs;
  uint64_t* msz;
  uint64_t* head;
};

__global__ __launch_bounds__(kThreads) void okv_split_layout_kernel(SplitLayoutParams P) {
  const uint64_t s = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (s >= P.S) return;
  const uint64_t b0 = P.fb[s], b1 = P.fb[s + 1];
  const SplitBytePre B{P.desc, P.nb, P.data_bytes};
  const SplitEntPre E{P.moff, P.nb, P.head_whole, P.meta_ent};
  const uint64_t r0 = P.first[b0], r1 = P.first[b1];
  const uint64_t head = split::meta_head(P.key_len[r0], P.key_len[r1 - 1], P.bloom_bytes);
  okv_split_seg g;
  g.first_row = r0;
  g.n_rows = r1 - r0;
  g.first_block = b0;
  g.n_blocks = b1 - b0;
  g.data_off = B(b0);
  g.data_bytes = B(b1) - g.data_off;
  g.meta_off = 0;  // (S6, after the scan)
  g.meta_bytes = head + E(b1) - E(b0);
  g.meta_hash = 0;  // (S10)
  g.file_bytes = g.data_bytes + g.meta_bytes + 25;
  P.segs[s] = g;
  P.msz[s] = split::round16(g.meta_bytes + 25);
  P.head[s] = head;
}

struct SplitMetaParams {
  const uint8_t* key_arena;
  const uint64_t* key_off;
  const uint16_t* key_len;
  const uint64_t* first;
  const Desc* desc;
  const uint64_t* hash;
  const uint64_t* moff;
  uint64_t nb, head_whole;
  const uint32_t* mark;
  const uint32_t* xl;
  const uint64_t* tile_pre;
  okv_split_seg* segs;
  const uint64_t* seg_moff;
  const uint64_t* seg_head;
  Desc* rdesc;
  Desc* hdesc;
  uint8_t* meta;
  uint64_t bloom_bytes;
  int comp_byte;
};

__global__ __launch_bounds__(kThreads) void okv_split_meta_kernel(SplitMetaParams P) {
  const uint64_t k = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (k >= P.nb) return;
  const uint32_t starts = P.mark[k];
  const uint64_t s = P.tile_pre[k / kETile] + P.xl[k] + starts - 1;
  const uint64_t mo = P.seg_moff[s], head = P.seg_head[s];
  const uint64_t b0 = P.segs[s].first_block, doff = P.segs[s].data_off;
  if (starts) {  // generateMetaBlock head (:288-325) of segment s
    const uint64_t r0 = P.segs[s].first_row, rz = r0 + P.segs[s].n_rows - 1;
    uint8_t* p = P.meta + mo;
    const uint32_t k0 = P.key_len[r0], kz = P.key_len[rz];
    put_le(p, k0, 2);
    put_bytes(p + 2, P.key_arena + P.key_off[r0], k0);
    p += 2 + k0;
    put_le(p, kz, 2);
    put_bytes(p + 2, P.key_arena + P.key_off[rz], kz);
    p += 2 + kz;
    if (P.bloom_bytes) {  // (the filter's bytes: S8)
      p[0] = 1;
      put_le(p + 1, P.bloom_bytes, 8);
      p += 9 + P.bloom_bytes;
    } else {
      p[0] = 0;
      p += 1;
    }
    p[0] = uint8_t(P.comp_byte);
    p[1] = 0;  // not a partitioned block index
    put_le(p + 2, P.segs[s].n_blocks, 8);
    P.segs[s].meta_off = mo;
    Desc h;
    h.offset = mo;
    h.block_size = P.segs[s].meta_bytes;
    h.original_size = h.compressed_size = 0;
    P.hdesc[s] = h;
  }
  // BlockStat.toBytes (block_stat.go:27-42) at its place in the segment's meta block
  uint8_t* p = P.meta + mo + head + (P.moff[k] - P.moff[b0]);
  const uint64_t r = P.first[k];
  const uint32_t kl = P.key_len[r];
  put_le(p, kl, 2);
  put_bytes(p + 2, P.key_arena + P.key_off[r], kl);
  p += 2 + kl;
  Desc d = P.desc[k];
  d.offset -= doff;
  P.rdesc[k] = d;
  put_le(p, d.offset, 8);
  put_le(p + 8, d.block_size, 8);
  put_le(p + 16, d.original_size, 8);
  put_le(p + 24, d.compressed_size, 8);
  put_le(p + 32, P.hash[k], 8);
}

// Add(key) of every row into its segment's filter: words + s * wps.
__global__ __launch_bounds__(kThreads) void okv_split_bloom_add_kernel(
    const uint8_t* __restrict__ key_arena, const uint64_t* __restrict__ key_off,
    const uint16_t* __restrict__ key_len, uint64_t n, const okv_split_seg* __restrict__ segs,
    uint64_t S, uint64_t* __restrict__ words, uint64_t wps, bloom::Modulus mod, uint32_t k) {
  for (uint64_t row = uint64_t(blockIdx.x) * kThreads + threadIdx.x; row < n;
       row += uint64_t(gridDim.x) * kThreads) {
    uint64_t lo = 0, hi = S - 1;  // the last segment with first_row <= row
    for (int it = 0; it < 64 && lo < hi; ++it) {
      const uint64_t mid = lo + (hi - lo + 1) / 2;
      if (segs[mid].first_row <= row)
        lo = mid;
      else
        hi = mid - 1;
    }
    uint64_t h[4];
    bloom::base_hashes(key_arena + key_off[row], key_len[row], h);
    uint64_t* w = words + lo * wps;
    for (uint32_t i = 0; i < k; ++i) {
      const uint64_t loc = bloom::location(h, i, mod);  // < m <= 64 wps
      atomicOr(reinterpret_cast<unsigned long long*>(w + (loc >> 6)), 1ull << (loc & 63));
    }
  }
}

// BloomFilter.WriteTo of every segment's filter (big-endian m, k, length, then the words)
// into its meta block at head - 10 - bloom_bytes: byte stores, any alignment.
__global__ __launch_bounds__(kThreads) void okv_split_bloom_write_kernel(
    const uint64_t* __restrict__ words, uint64_t wps, uint64_t S, uint64_t m, uint64_t k,
    const uint64_t* __restrict__ seg_moff, const uint64_t* __restrict__ seg_head,
    uint8_t* __restrict__ meta) {
  const uint64_t per = wps + 3, bloom_bytes = 8 * per;
  for (uint64_t x = uint64_t(blockIdx.x) * kThreads + threadIdx.x; x < S * per;
       x += uint64_t(gridDim.x) * kThreads) {
    const uint64_t s = x / per, i = x - s * per;
    const uint64_t v = i == 0 ? m : i == 1 ? k : i == 2 ? m : words[s * wps + i - 3];
    uint8_t* p = meta + seg_moff[s] + seg_head[s] - 10 - bloom_bytes + 8 * i;
    for (int b = 0; b < 8; ++b) p[b] = uint8_t(v >> (8 * (7 - b)));
  }
}

// Close per segment: the trailer (trailer_bytes' layout) after the meta block, its meta
// offset the segment's own data length; the arena's padding up to 16 bytes zeroed.
__global__ __launch_bounds__(kThreads) void okv_split_trailer_kernel(
    okv_split_seg* __restrict__ segs, uint64_t S, const uint64_t* __restrict__ mhash,
    uint8_t* __restrict__ meta) {
  const uint64_t s = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (s >= S) return;
  const uint64_t h = mhash[s];
  segs[s].meta_hash = h;
  const uint64_t mb = segs[s].meta_bytes;
  uint8_t* t = meta + segs[s].meta_off + mb;
  put_le(t, segs[s].data_bytes, 8);
  put_le(t + 8, h, 8);
  t[16] = 1;
  put_le(t + 17, 69696969696969ULL, 8);
  for (uint64_t i = mb + 25; i < split::round16(mb + 25); ++i) t[i - mb] = 0;
}

namespace {

int read_split_totals(okv_ctx* ctx, EncScratch* e) {
  OKV_HIP(hipMemcpyAsync(e->sp_htot.data(), e->sp_dtot.data(), 2 * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, ctx->stream));
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  return OKV_OK;
}

// S1-S5: the segments of the plan in e.  *S and *arena: their number and the meta arena's
// bytes.  Two host synchronisations.
int split_group(okv_ctx* ctx, EncScratch* e, const DevRows& R, const Plan& pl,
                const okv_split_opts& so, uint64_t bloom_bytes, uint64_t* S, uint64_t* arena) {
  const uint64_t nb = pl.nb, c = nb + 1;
  const uint32_t nbt = ceil_div(nb, kETile);
  int rc;
  if ((rc = reserve(ctx, e->sp_j[0], c)) || (rc = reserve(ctx, e->sp_j[1], c)) ||
      (rc = reserve(ctx, e->sp_mark, c)) || (rc = reserve(ctx, e->sp_xl, c)) ||
      (rc = reserve(ctx, e->sp_ttot, nbt + 1)) || (rc = reserve(ctx, e->sp_tpre, nbt + 1)) ||
      (rc = reserve(ctx, e->sp_fb, c)) || (rc = reserve(ctx, e->sp_dtot, 2)) ||
      (rc = reserve(ctx, e->sp_htot, 2)))
    return rc;
  const uint32_t gb = ceil_div(c, kThreads);
  hipLaunchKernelGGL(okv_split_next_kernel, dim3(gb), dim3(kThreads), 0, ctx->stream,
                     e->desc.data(), e->first.data(), nb, pl.data_bytes, so.split_bytes,
                     so.split_rows, e->sp_j[0].data(), e->sp_mark.data());
  const uint32_t rounds = split::rounds(nb);
  for (uint32_t k = 0; k < rounds; ++k)
    hipLaunchKernelGGL(okv_split_jump_kernel, dim3(gb), dim3(kThreads), 0, ctx->stream,
                       e->sp_j[k & 1].data(), e->sp_j[(k + 1) & 1].data(), e->sp_mark.data(), nb);
  hipLaunchKernelGGL(okv_split_number_kernel, dim3(nbt), dim3(kThreads), 0, ctx->stream,
                     e->sp_mark.data(), nb, e->sp_xl.data(), e->sp_ttot.data());
  hipLaunchKernelGGL(okv_enc_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, e->sp_ttot.data(),
                     uint64_t(nbt), e->sp_tpre.data(), e->sp_dtot.data());
  hipLaunchKernelGGL(okv_split_start_kernel, dim3(ceil_div(nb, kThreads)), dim3(kThreads), 0,
                     ctx->stream, e->sp_mark.data(), e->sp_xl.data(), e->sp_tpre.data(), nb,
                     e->sp_dtot.data(), e->sp_fb.data());
  OKV_HIP(hipGetLastError());
  if ((rc = read_split_totals(ctx, e))) return rc;
  const uint64_t ns = e->sp_htot.data()[0];
  if (ns == 0 || ns > nb) return set_err(ctx, OKV_E_HIP, "split: inconsistent segment count");
  if ((rc = reserve(ctx, e->sp_segs, ns)) || (rc = reserve(ctx, e->sp_msz, ns)) ||
      (rc = reserve(ctx, e->sp_moff, ns)) || (rc = reserve(ctx, e->sp_head, ns)) ||
      (rc = reserve(ctx, e->sp_mhash, ns)) || (rc = reserve(ctx, e->sp_hdesc, ns)) ||
      (rc = reserve(ctx, e->sp_rdesc, nb)))
    return rc;
  SplitLayoutParams lp;
  lp.fb = e->sp_fb.data();
  lp.S = ns;
  lp.nb = nb;
  lp.desc = e->desc.data();
  lp.first = e->first.data();
  lp.moff = e->moff.data();
  lp.key_len = R.kl;
  lp.data_bytes = pl.data_bytes;
  lp.meta_ent = pl.meta_bytes - pl.head;
  lp.head_whole = pl.head;
  lp.bloom_bytes = bloom_bytes;
  lp.segs = e->sp_segs.data();
  lp.msz = e->sp_msz.data();
  lp.head = e->sp_head.data();
  hipLaunchKernelGGL(okv_split_layout_kernel, dim3(ceil_div(ns, kThreads)), dim3(kThreads), 0,
                     ctx->stream, lp);
  hipLaunchKernelGGL(okv_enc_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, e->sp_msz.data(),
                     ns, e->sp_moff.data(), e->sp_dtot.data() + 1);
  OKV_HIP(hipGetLastError());
  if ((rc = read_split_totals(ctx, e))) return rc;
  *S = ns;
  *arena = e->sp_htot.data()[1];
  return OKV_OK;
}

}  // namespace
}  // namespace okv

extern "C" int okv_encode_split(okv_ctx* ctx, const okv_rows* rows, const okv_encode_opts* opts,
                                const okv_split_opts* split, okv_split_out* out, uint32_t flags) {
  if (!ctx || !rows || !opts || !split || !out) return OKV_E_ARG;
  out->n_segments = out->n_blocks = out->data_bytes = out->meta_arena_bytes = 0;
  out->bad_row = kNone;
  if (flags & ~uint32_t(OKV_F_DEVICE_PTRS))
    return set_err(ctx, OKV_E_ARG, "split: flags other than OKV_F_DEVICE_PTRS");
  if (opts->strict_go)
    return set_err(ctx, OKV_E_ARG, "split: strict_go (a segment closes right after a flush, Q1)");
  if (opts->bloom) return set_err(ctx, OKV_E_ARG, "split: opts->bloom (the filters are the call's)");
  if (opts->compression != OKV_COMP_NONE && opts->compression != OKV_COMP_LZ4)
    return set_err(ctx, OKV_E_ARG, "split: compression");
  if (opts->block_size == 0) return set_err(ctx, OKV_E_ARG, "block_size == 0");
  if (split->bloom_k > 4096) return set_err(ctx, OKV_E_ARG, "bloom: k > 4096");
  const uint64_t n = rows->n_rows;
  if (n == 0) return set_err(ctx, OKV_W_NO_ROWS, "ErrNoRowsWritten");
  if (n >= (uint64_t(1) << 32) - kETile) return set_err(ctx, OKV_E_ARG, "n_rows >= 2^32");
  if (!rows->key_off || !rows->key_len || !rows->val_off || !rows->val_len ||
      (!rows->key_arena && rows->key_arena_bytes) || (!rows->val_arena && rows->val_arena_bytes))
    return set_err(ctx, OKV_E_ARG, "rows");
  const bool dev = flags & OKV_F_DEVICE_PTRS;
  if (dev && (reinterpret_cast<uintptr_t>(out->meta) & 15))
    return set_err(ctx, OKV_E_ARG, "split: device meta is not 16-byte aligned");
  // bloom.New: max(1, m), max(1, k); WriteTo: 24 bytes + the words
  const uint64_t bm = std::max<uint64_t>(1, split->bloom_m), bk = split->bloom_k;
  if (bk && bm > (uint64_t(1) << 40)) return set_err(ctx, OKV_E_ARG, "bloom: m > 2^40");
  const uint64_t wps = bk ? (bm + 63) >> 6 : 0;
  const uint64_t bloom_bytes = bk ? 24 + 8 * wps : 0;
  OKV_HIP(hipSetDevice(ctx->device));
  EncScratch* e;
  int rc = enc_scratch(ctx, &e);
  if (rc) return rc;
  DevRows R;
  R.n = n;
  if ((rc = rows_on_device(ctx, e, rows, dev, &R))) return rc;
  Plan pl;
  uint64_t bad = kNone;
  rc = enc_plan(ctx, e, R, *opts, &pl, &bad);
  ctx->last_path = 0;
  if (rc == OKV_W_INVALID_KEY) out->bad_row = bad;
  if (rc) return rc;
  uint64_t S = 0, arena = 0;
  if ((rc = split_group(ctx, e, R, pl, *split, bloom_bytes, &S, &arena))) return rc;
  out->n_segments = S;
  out->n_blocks = pl.nb;
  out->data_bytes = pl.data_bytes;
  out->meta_arena_bytes = arena;
  const bool want_idx = out->blk_first_row || out->blk_desc || out->blk_hash;
  if (out->data_cap < pl.data_bytes || out->meta_cap < arena || out->seg_cap < S ||
      (want_idx && out->blk_cap < pl.nb) || !out->data || !out->meta || !out->segs)
    return set_err(ctx, OKV_E_CAPACITY, "split output capacity too small (sizes set)");
  if (bk && S * wps > (uint64_t(1) << 37))
    return set_err(ctx, OKV_E_ARG, "split: the segments' filters exceed 1 TiB");
  uint8_t *data = out->data, *meta = out->meta;
  if (!dev) {
    if ((rc = reserve(ctx, e->d_outseg, pl.data_bytes + 64)) ||
        (rc = reserve(ctx, e->sp_meta, arena + 64)))
      return rc;
    data = e->d_outseg.data();
    meta = e->sp_meta.data();
  }
  // data blocks and their hashes: the encoder's pack stage over the whole row list
  bool hashed = false, fk_done = false;
  if ((rc = enc_pack(ctx, e, R, *opts, pl, data, pack_params(e, R, data), &hashed, &fk_done)))
    return rc;
  if (!hashed)
    launch_hash(ctx->stream, data, pl.data_bytes, e->desc.data(), uint32_t(pl.nb), e->hash.data());
  SplitMetaParams mp;
  mp.key_arena = R.ka;
  mp.key_off = R.ko;
  mp.key_len = R.kl;
  mp.first = e->first.data();
  mp.desc = e->desc.data();
  mp.hash = e->hash.data();
  mp.moff = e->moff.data();
  mp.nb = pl.nb;
  mp.head_whole = pl.head;
  mp.mark = e->sp_mark.data();
  mp.xl = e->sp_xl.data();
  mp.tile_pre = e->sp_tpre.data();
  mp.segs = e->sp_segs.data();
  mp.seg_moff = e->sp_moff.data();
  mp.seg_head = e->sp_head.data();
  mp.rdesc = e->sp_rdesc.data();
  mp.hdesc = e->sp_hdesc.data();
  mp.meta = meta;
  mp.bloom_bytes = bloom_bytes;
  mp.comp_byte = opts->compression == OKV_COMP_LZ4 ? 2 : 0;
  hipLaunchKernelGGL(okv_split_meta_kernel, dim3(ceil_div(pl.nb, kThreads)), dim3(kThreads), 0,
                     ctx->stream, mp);
  if (bk) {
    if ((rc = reserve(ctx, e->sp_words, S * wps))) return rc;
    OKV_HIP(hipMemsetAsync(e->sp_words.data(), 0, S * wps * 8, ctx->stream));
    const uint32_t cap = cu_count(ctx) * 8;
    hipLaunchKernelGGL(okv_split_bloom_add_kernel,
                       dim3(std::max<uint32_t>(1, std::min<uint32_t>(ceil_div(n, kThreads), cap))),
                       dim3(kThreads), 0, ctx->stream, R.ka, R.ko, R.kl, n, e->sp_segs.data(), S,
                       e->sp_words.data(), wps, bloom::modulus(bm), uint32_t(bk));
    const uint64_t items = S * (wps + 3);
    hipLaunchKernelGGL(okv_split_bloom_write_kernel,
                       dim3(uint32_t(std::min<uint64_t>((items + kThreads - 1) / kThreads,
                                                        uint64_t(cap) * 4))),
                       dim3(kThreads), 0, ctx->stream, e->sp_words.data(), wps, S, bm, bk,
                       e->sp_moff.data(), e->sp_head.data(), meta);
  }
  // Close on the device: XXH64 of every meta block, then the trailers
  launch_hash(ctx->stream, meta, arena, e->sp_hdesc.data(), uint32_t(S), e->sp_mhash.data());
  hipLaunchKernelGGL(okv_split_trailer_kernel, dim3(ceil_div(S, kThreads)), dim3(kThreads), 0,
                     ctx->stream, e->sp_segs.data(), S, e->sp_mhash.data(), meta);
  OKV_HIP(hipGetLastError());
  const hipMemcpyKind k = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  OKV_HIP(hipMemcpyAsync(out->segs, e->sp_segs.data(), S * sizeof(okv_split_seg), k, ctx->stream));
  if (out->blk_first_row)
    OKV_HIP(hipMemcpyAsync(out->blk_first_row, e->first.data(), (pl.nb + 1) * 8, k, ctx->stream));
  if (out->blk_desc)
    OKV_HIP(hipMemcpyAsync(out->blk_desc, e->sp_rdesc.data(), pl.nb * sizeof(Desc), k,
                           ctx->stream));
  if (out->blk_hash)
    OKV_HIP(hipMemcpyAsync(out->blk_hash, e->hash.data(), pl.nb * 8, k, ctx->stream));
  if (!dev) {
    OKV_HIP(hipMemcpyAsync(out->data, data, pl.data_bytes, k, ctx->stream));
    OKV_HIP(hipMemcpyAsync(out->meta, meta, arena, k, ctx->stream));
  }
  OKV_HIP(hipStreamSynchronize(ctx->stream));
  return OKV_OK;
}
