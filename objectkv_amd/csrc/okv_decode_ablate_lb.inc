// Ablation build only (#included by okv_decode.hip under -DOKV_ABLATE, in
// namespace okv): the single-pass small-block decode with a decoupled
// look-back (okv_decode_stream_kernel, OKV_DECODE_STREAM=1), measured slower
// than passes 1-3 (DESIGN.md 13.5).

// The look-back arm of fused_pass (kLB = true).
__device__ Prefix fused_prefix_lookback(const CopyParams& P, const FusedParams& F, uint32_t b,
                                        uint32_t lane, uint32_t tag, const Prefix& mine) {
  Prefix ex{0, 0, 0, 0};
  // ---- pass 2 by decoupled look-back: publish this block's aggregate,
  // then read the flags of the 64 blocks before it at once (one lane each),
  // waiting until each has published at least its aggregate; the nearest
  // inclusive prefix in the window ends the look-back, else the window's
  // aggregates are added and the next 64 are read.  Blocks take their
  // index from a counter in start order, so every block waited on is
  // running: any batch size is safe.
  if (lane == 0) {
    publish(&F.flag[b], &F.agg[b], mine, tag | 1u);
    atomicAdd(F.arr, 1ull);  // (kept in step with F.ctr: the host's base)
  }
  int64_t hi = int64_t(b) - 1;
  for (;;) {
    const int64_t k = hi - int64_t(lane);
    uint32_t f = k >= 0 ? flag_peek(&F.flag[k]) : (tag | 2u);
    while (__any((f & ~3u) != tag)) {
      __builtin_amdgcn_s_sleep(1);
      if ((f & ~3u) != tag) f = flag_peek(&F.flag[k]);
    }
    const uint64_t inc = __ballot((f & 3u) == 2u);
    const uint32_t j = inc ? uint32_t(__ffsll(static_cast<unsigned long long>(inc)) - 1) : 64u;
    // lanes < j: aggregates; lane j: an inclusive prefix (zero before block 0)
    Prefix v{0, 0, 0, 0};
    if (lane < j && k >= 0) v = prefix_peek(&F.agg[k]);
    if (lane == j && k >= 0) v = prefix_peek(&F.incl[k]);
    ex.rows += wave_sum64(v.rows);
    ex.kb += wave_sum64(v.kb);
    ex.vb += wave_sum64(v.vb);
    ex.bad += wave_sum64(v.bad);
    if (j < 64) break;
    hi -= 64;
  }
  if (lane == 0) {  // this block's inclusive prefix
    const Prefix in{ex.rows + mine.rows, ex.kb + mine.kb, ex.vb + mine.vb, ex.bad + mine.bad};
    publish(&F.flag[b], &F.incl[b], in, tag | 2u);
    if (b == P.nblk - 1) {
      *F.tot = Totals{in.rows, in.kb, in.vb, in.bad};
      P.row_start[P.nblk] = in.rows;
    }
  }
  return ex;
}

// Ablation build (OKV_DECODE_STREAM=1): single pass for batches of small
// blocks of any size (> kFusedMaxBlocks), the fused kernel's per-block work
// with the prefix by decoupled look-back.  Each block is read once, but one
// block per workgroup makes the look-back chase a frontier that lags by the
// workgroups in flight (CM: 9.2 vs 1.38 ms for passes 1-3, profiles/r4).
__global__ __launch_bounds__(64) void okv_decode_stream_kernel(CopyParams P, FusedParams F) {
  fused_pass<true>(P, F);
}


// ---------------------------------------------------------------------------
// Ablation arm OKV_VALUE_SWEEP=9 (round 5): the whole large-block decode in
// one launch, one workgroup per block.  The block (<= 64 KiB) is DMA'd into
// LDS, lane 0 walks its headers there (okv_count_kernel's checks), the block
// publishes its counts and takes its exclusive prefix by a decoupled
// look-back over the NT blocks before it at once (one thread each), then
// writes its SoA rows and arena regions from LDS (emit_fast; materialise
// past kFastRows rows).  No count kernel, no header walk in HBM.  Blocks
// claim their index from a counter in start order, so every block waited on
// is running.  Blocks larger than the stage walk and copy from HBM.
// ---------------------------------------------------------------------------
template <uint32_t NT>
__device__ Prefix block_lookback(const FusedParams& F, uint32_t b, uint32_t tag) {
  __shared__ Prefix s_red[NT / 64];
  __shared__ uint32_t s_j[NT / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Prefix ex{0, 0, 0, 0};
  int64_t hi = int64_t(b) - 1;
  for (;;) {
    const int64_t k = hi - int64_t(tid);  // thread t reads block hi - t
    uint32_t f = k >= 0 ? flag_peek(&F.flag[k]) : (tag | 2u);
    while ((f & ~3u) != tag) {  // not yet published this call: wait for its aggregate
      __builtin_amdgcn_s_sleep(1);
      f = flag_peek(&F.flag[k]);
    }
    const uint64_t inc = __ballot((f & 3u) == 2u);
    if (lane == 0)
      s_j[wave] = inc ? wave * 64 + uint32_t(__ffsll(static_cast<unsigned long long>(inc)) - 1)
                      : 0xffffffffu;
    __syncthreads();
    uint32_t J = 0xffffffffu;  // the nearest inclusive prefix in the window
#pragma unroll
    for (uint32_t w = 0; w < NT / 64; ++w) J = min(J, s_j[w]);
    Prefix v{0, 0, 0, 0};
    if (k >= 0 && tid < J) v = prefix_peek(&F.agg[k]);
    if (k >= 0 && tid == J) v = prefix_peek(&F.incl[k]);
    v.rows = wave_sum64(v.rows);
    v.kb = wave_sum64(v.kb);
    v.vb = wave_sum64(v.vb);
    v.bad = wave_sum64(v.bad);
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t w = 0; w < NT / 64; ++w) {
      ex.rows += s_red[w].rows;
      ex.kb += s_red[w].kb;
      ex.vb += s_red[w].vb;
      ex.bad += s_red[w].bad;
    }
    __syncthreads();  // s_j / s_red reuse
    if (J != 0xffffffffu) break;
    hi -= int64_t(NT);
  }
  return ex;
}

// kLB = false (OKV_VALUE_SWEEP=11, diagnostic): the prefix from okv_count_kernel
// (which runs first), block b = blockIdx.x -- the per-block decode's cost
// without the look-back wait.
template <uint32_t NT, bool kLB = true>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(NT == 1024 ? 8 : 4))) void
okv_block_kernel(CopyParams P, FusedParams F) {
  __shared__ CopySmem sm;
  __shared__ uint64_t s_walk[4];
  __shared__ int32_t s_st;
  __shared__ uint32_t s_b;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_b = kLB ? uint32_t(atomicAdd(F.ctr, 1ull) - F.base) : blockIdx.x;
  __syncthreads();
  const uint32_t b = __builtin_amdgcn_readfirstlane(s_b);
  if (b >= P.nblk) return;
  const uint32_t tag = F.epoch << 2;
  const Desc d = P.descs[b];
  const int32_t st0 = go_read_status(d, P.seg_bytes);  // :303-316
  const uint64_t len = P.comp == OKV_COMP_LZ4 ? 0 : d.block_size;  // Q7 (:331-333)
  const uint64_t off = d.offset;
  const bool staged = st0 == OKV_BLK_OK && len <= uint64_t(kStage);
  // stage = segment lines [A, E): the line before the block's first byte
  // through the line after its last (16-byte guards for the funnels)
  const int64_t A = int64_t(off & ~uint64_t(15)) - 16;
  const uint32_t bias = uint32_t(int64_t(off) - A);
  if (staged && len && tid >= 64) {  // waves 1.. DMA; wave 0 walks once they land
    const int64_t E = int64_t((off + len + 15) & ~uint64_t(15)) + 16;
    const uint32_t np = uint32_t((E - A) >> 4);
    const int64_t lim = int64_t(round16(P.seg_bytes));
    const uint32_t u = tid - 64;
    for (uint32_t k0 = 0; k0 < np; k0 += NT - 64) {
      const uint32_t i = k0 + u;
      if (i < np) {
        int64_t a = A + (int64_t(i) << 4);
        if (a < 0 || a + 16 > lim) a = int64_t(off) & ~int64_t(15);  // bytes never used
        __builtin_amdgcn_global_load_lds(P.seg + a, OKV_LDS_PTR(sm.stage + k0 + (u & ~63u)), 16,
                                         0, 0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  if (tid == 0) {  // the walk (okv_count_kernel's checks in Go's order, :338-352)
    int32_t st = st0;
    uint64_t rows = 0, kb = 0, vb = 0, p = 0;
    if (st == OKV_BLK_OK) {
      const uint64_t orig = go_walk_bound(d.original_size);  // :340
      const uint32_t* sw = reinterpret_cast<const uint32_t*>(sm.stage);
      while (p < orig) {
        if (len - p < 6) { st = OKV_BLK_PANIC; break; }  // :342-345
        uint32_t kl, vl;
        if (staged)
          header_lds(sw, bias + uint32_t(p), kl, vl);
        else
          header_global(P.seg, off + p, kl, vl);
        const uint64_t room = len - p - 6;
        if (kl > room || vl > room - kl) { st = OKV_BLK_PANIC; break; }  // :346-349
        if (rows < uint64_t(kFastRows)) {
          sm.f.rec[rows] = uint32_t(p);
          sm.f.kpre[rows] = uint32_t(kb);
          sm.f.vpre[rows] = uint32_t(vb);
        }
        rows++;
        kb += kl;
        vb += vl;
        p += 6 + uint64_t(kl) + uint64_t(vl);
      }
      if (st == OKV_BLK_OK && rows <= uint64_t(kFastRows)) {
        sm.f.rec[rows] = uint32_t(p);
        sm.f.kpre[rows] = uint32_t(kb);
        sm.f.vpre[rows] = uint32_t(vb);
      }
    }
    if (st != OKV_BLK_OK) rows = kb = vb = p = 0;
    s_walk[0] = rows;
    s_walk[1] = kb;
    s_walk[2] = vb;
    s_walk[3] = p;
    s_st = st;
    if (kLB) {
      const Prefix mine{rows, round16(kb), round16(vb), uint64_t(st != OKV_BLK_OK)};
      publish(&F.flag[b], &F.agg[b], mine, tag | 1u);
      atomicAdd(F.arr, 1ull);  // (kept in step with F.ctr: the host's base)
    }
  }
  __syncthreads();
  const uint64_t rows = s_walk[0], kb = s_walk[1], vb = s_walk[2], pend = s_walk[3];
  const Prefix ex = kLB ? block_lookback<NT>(F, b, tag) : Prefix{P.lp[b].rows + P.tile_pre[b / kTile].rows,
      P.lp[b].kb + P.tile_pre[b / kTile].kb, P.lp[b].vb + P.tile_pre[b / kTile].vb,
      P.lp[b].bad + P.tile_pre[b / kTile].bad};
  if (kLB && tid == 0) {
    const Prefix in{ex.rows + rows, ex.kb + round16(kb), ex.vb + round16(vb),
                    ex.bad + uint64_t(s_st != OKV_BLK_OK)};
    publish(&F.flag[b], &F.incl[b], in, tag | 2u);
    if (b == P.nblk - 1) {
      *F.tot = Totals{in.rows, in.kb, in.vb, in.bad};
      P.row_start[P.nblk] = in.rows;
    }
  }
  BlockCount c{rows, kb, vb, pend, s_st, 0};
  const BlockBase B = block_base_of(P, c, ex, Prefix{0, 0, 0, 0});
  if (tid == 0) {
    P.row_start[b] = B.row0;
    P.key_base[b] = B.kb0;
    P.val_base[b] = B.vb0;
    P.blk_status[b] = B.st;
  }
  if (B.st != OKV_BLK_OK || rows == 0) return;
  if (staged && rows <= uint64_t(kFastRows)) {
    emit_fast(P, sm, bias, int(rows), kb, vb, B.row0, B.kb0, B.vb0);
  } else if (staged) {
    const Staged src{sm.stage, bias};
    materialise(src, P, sm, rows, kb, vb, B.row0, B.kb0, B.vb0, pend);
  } else {
    GlobalSrc src{P.seg, P.seg_bytes, off};
    materialise(src, P, sm, rows, kb, vb, B.row0, B.kb0, B.vb0, pend);
  }
}

// ---------------------------------------------------------------------------
// Ablation build (OKV_DECODE_GROUP=1).  Single-pass decode of large batches of
// small blocks (OKV_PATH_GROUP; the CM
// compaction feed's 386 K x 4 KiB segments): each block's bytes are read from
// HBM once.  One 256-thread workgroup per group of kGroup consecutive blocks:
//   1. every wave DMAs its four blocks into their LDS slots (64 KiB of the
//      group in flight at once) and walks their headers there (walk_staged_to,
//      Go's checks in Go's order);
//   2. the group's counts go out as an aggregate, and wave 0 sums its
//      predecessors' by a decoupled look-back over 64 groups per round
//      (aggregate / inclusive flags tagged with the call's epoch; write-
//      through payloads drained before their flag, read with sc1 loads after
//      it -- the fused kernel's hand-off);
//   3. every wave gathers its blocks' rows from their slots.
// The prefix is what okv_count_kernel + its scan would give, so outputs are
// identical to the two-pass form (count, then okv_gather_small_kernel
// re-reading every block).  With kGroup blocks per look-back entry the
// frontier spans 64 x kGroup blocks per round trip; round 4's one-block-per-
// workgroup stream kernel advanced 64 blocks per round trip (DESIGN.md 13.5).
// Blocks past the slot take the HBM walk and gather; blocks of more than
// kRCap rows go on the big-block list (okv_copy_kernel) as from pass 1.
#ifndef OKV_GROUP_BLOCKS  // (A/B builds: tools/build_dec_variant.sh -DOKV_GROUP_BLOCKS=8)
#define OKV_GROUP_BLOCKS 16
#endif
constexpr uint32_t kGroup = OKV_GROUP_BLOCKS;  // blocks per workgroup (kGroup / 4 per wave)
constexpr uint32_t kGroupPerWave = kGroup / 4;
static_assert(kGroup % 4 == 0 && kGroup <= 64, "whole blocks per wave");
constexpr uint32_t kGroupSlot = 4160;   // staged bytes per block: a 4 KiB block + lead-in + slack
struct GroupParams {
  const int32_t* pre;  // zstd-stage statuses or null
  BlockCount* cnt;     // what passes 1-2 write, for okv_copy_kernel
  Prefix* lp;
  Prefix* tile_pre;
  uint32_t* flag;      // [group] (epoch << 2) | 1 aggregate published, | 2 inclusive
  Prefix* agg;         // [group]
  Prefix* incl;        // [group] inclusive prefix
  uint32_t epoch;      // per call, never 0 (the flags start zeroed)
  Totals* tot;
  uint32_t* big_zero;  // the other big-block counter slot: zeroed for the next launch
};
struct __align__(16) GroupSmem {
  uint4 stage[kGroup][kGroupSlot / 16];
  uint32_t rec[kGroup][kRCap + 1];
  GatherSmem g[4];                 // row tables, one per wave
  uint64_t cnt[kGroup][4];         // rows, key bytes, value bytes, walk end
  uint64_t off[kGroup];
  int32_t st[kGroup];
  uint32_t staged[kGroup];
  Prefix loc[kGroup];              // exclusive prefix within the group
  Prefix ex;                       // the group's exclusive prefix
};

__global__ __launch_bounds__(kThreads) void okv_group_kernel(CopyParams P, GroupParams G) {
  __shared__ GroupSmem sm;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t g = blockIdx.x, b0 = g * kGroup;
  const uint32_t nb = min(kGroup, P.nblk - b0);
  if (g == 0 && tid == 0) *G.big_zero = 0;
  // ---- 1. descriptors, statuses, the DMA of the wave's blocks ----
  const int64_t lim = int64_t(round16(P.seg_bytes));
#pragma unroll
  for (uint32_t i = 0; i < kGroupPerWave; ++i) {
    const uint32_t lb = wave * kGroupPerWave + i;
    if (lb >= nb) break;
    const uint32_t b = b0 + lb;
    const Desc d = P.descs[b];
    uint64_t len;
    const int32_t st = entry_status(d, P.seg_bytes, P.comp, G.pre, b, len);
    const uint32_t shift = uint32_t(d.offset & 15);
    const bool staged = st == OKV_BLK_OK && len + 16 + shift + 32 <= kGroupSlot;
    if (lane == 0) {
      sm.off[lb] = d.offset;
      sm.st[lb] = st;
      sm.staged[lb] = staged;
    }
    if (staged && len) {  // [offset - shift - 16, offset + len + 32) into the slot
      const int64_t D = int64_t(d.offset) - int64_t(shift) - 16;
      const uint32_t n16 = uint32_t((16 + shift + len + 32 + 15) >> 4);
      for (uint32_t c0 = 0; c0 < n16; c0 += 64) {
        if (c0 + lane < n16) {  // (an inactive lane writes no LDS)
          int64_t a = D + (int64_t(c0 + lane) << 4);
          if (a < 0 || a + 16 > lim) a = int64_t(d.offset) & ~int64_t(15);  // bytes never used
          __builtin_amdgcn_global_load_lds(P.seg + a, OKV_LDS_PTR(&sm.stage[lb][c0]), 16, 0, 0);
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // ---- the walks (each wave its own blocks: its own DMA, so no barrier) ----
#pragma unroll
  for (uint32_t i = 0; i < kGroupPerWave; ++i) {
    const uint32_t lb = wave * kGroupPerWave + i;
    if (lb >= nb) break;
    const Desc d = P.descs[b0 + lb];
    int32_t st = sm.st[lb];
    uint64_t rows = 0, kb = 0, vb = 0, p = 0;
    const uint64_t len = (P.comp == OKV_COMP_LZ4) ? 0 : d.block_size;
    if (st == OKV_BLK_OK && sm.staged[lb]) {
      const Staged lsrc{&sm.stage[lb][0], 16 + uint32_t(d.offset & 15)};
      walk_staged_to(lsrc, uint32_t(len), d.original_size, RecSink{sm.rec[lb], kRCap}, lane, st,
                     rows, kb, vb, p);
    } else if (st == OKV_BLK_OK) {
      walk_global(P.seg, d.offset, len, d.original_size, sm.rec[lb], lane, st, rows, kb, vb, p);
    }
    if (lane == 0) {
      sm.st[lb] = st;
      sm.cnt[lb][0] = rows;
      sm.cnt[lb][1] = kb;
      sm.cnt[lb][2] = vb;
      sm.cnt[lb][3] = p;
    }
  }
  __syncthreads();
  // ---- 2. the group's prefix (wave 0) ----
  if (wave == 0) {
    const bool live = lane < nb;
    uint64_t v[4] = {live ? sm.cnt[lane][0] : 0, live ? round16(sm.cnt[lane][1]) : 0,
                     live ? round16(sm.cnt[lane][2]) : 0,
                     uint64_t(live && sm.st[lane] != OKV_BLK_OK)};
    uint64_t inc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) inc[k] = wave_incl_scan(v[k], lane);
    if (live) sm.loc[lane] = Prefix{inc[0] - v[0], inc[1] - v[1], inc[2] - v[2], inc[3] - v[3]};
    const Prefix agg{__shfl(inc[0], 63, 64), __shfl(inc[1], 63, 64), __shfl(inc[2], 63, 64),
                     __shfl(inc[3], 63, 64)};
    const uint32_t tagA = (G.epoch << 2) | 1u, tagP = (G.epoch << 2) | 2u;
    if (lane == 0) publish(&G.flag[g], &G.agg[g], agg, tagA);
    Prefix ex{0, 0, 0, 0};
    for (int64_t k_hi = int64_t(g) - 1; k_hi >= 0; k_hi -= 64) {
      const int64_t k = k_hi - int64_t(lane);  // lane 0: the nearest predecessor
      uint32_t f = k >= 0 ? flag_peek(&G.flag[k]) : tagP;
      bool ready = k < 0 || f == tagA || f == tagP;
      while (__ballot(!ready)) {
        if (!ready) {
          __builtin_amdgcn_s_sleep(1);
          f = flag_peek(&G.flag[k]);
          ready = f == tagA || f == tagP;
        }
      }
      // the nearest inclusive prefix ends the look-back; the aggregates of
      // the groups after it are added to it
      const uint64_t pm = __ballot(k >= 0 && f == tagP);
      const uint32_t stop = pm ? uint32_t(__builtin_ctzll(pm)) : 64u;
      if (k >= 0 && lane <= stop) {
        const Prefix o = lane == stop ? prefix_peek(&G.incl[k]) : prefix_peek(&G.agg[k]);
        ex.rows += o.rows;
        ex.kb += o.kb;
        ex.vb += o.vb;
        ex.bad += o.bad;
      }
      if (pm) break;
    }
    ex.rows = wave_sum64(ex.rows);
    ex.kb = wave_sum64(ex.kb);
    ex.vb = wave_sum64(ex.vb);
    ex.bad = wave_sum64(ex.bad);
    const Prefix in{ex.rows + agg.rows, ex.kb + agg.kb, ex.vb + agg.vb, ex.bad + agg.bad};
    if (lane == 0) {
      publish(&G.flag[g], &G.incl[g], in, tagP);
      sm.ex = ex;
      if (g == gridDim.x - 1) {  // the totals
        *G.tot = Totals{in.rows, in.kb, in.vb, in.bad};
        P.row_start[P.nblk] = in.rows;
      }
    }
  }
  __syncthreads();
  // ---- 3. outputs and the gather, each wave its four blocks ----
  GatherSmem& gs = sm.g[wave];
#pragma unroll 1
  for (uint32_t i = 0; i < kGroupPerWave; ++i) {
    const uint32_t lb = wave * kGroupPerWave + i;
    if (lb >= nb) break;
    const uint32_t b = b0 + lb;
    const Prefix l = sm.loc[lb];
    const Prefix ex{sm.ex.rows + l.rows, sm.ex.kb + l.kb, sm.ex.vb + l.vb, sm.ex.bad + l.bad};
    BlockMeta m;
    m.c = BlockCount{sm.cnt[lb][0], sm.cnt[lb][1], sm.cnt[lb][2], sm.cnt[lb][3], sm.st[lb], 0};
    m.B = block_base_of(P, m.c, ex, Prefix{0, 0, 0, 0});
    m.off = sm.off[lb];
    const uint64_t rows = m.c.rows;
    if (lane == 0) {  // what passes 1-2 leave for okv_copy_kernel, and the block outputs
      G.cnt[b] = m.c;
      G.lp[b] = ex;
      if (b % kTile == 0) G.tile_pre[b / kTile] = Prefix{0, 0, 0, 0};
      if (m.c.status == OKV_BLK_OK && (rows > kRCap || m.c.pend >= (uint64_t(1) << 32)))
        P.big_list[atomicAdd(P.big_count, 1u)] = b;
      P.row_start[b] = m.B.row0;
      if (P.key_base) P.key_base[b] = m.B.kb0;
      if (P.val_base) P.val_base[b] = m.B.vb0;
      P.blk_status[b] = m.B.st;
    }
    if (!(m.B.st == OKV_BLK_OK && rows != 0 && rows <= uint64_t(kRCap) &&
          m.c.pend < (uint64_t(1) << 32)))
      continue;
    const int nr = int(rows);
    const uint32_t rec = int(lane) < nr ? sm.rec[lb][lane] : 0u;
    // the row index (lane r = row r)
    auto row_index = [&]() {
      if (int(lane) >= nr) return;
      const uint64_t gr = m.B.row0 + lane;
      const uint32_t kl = gs.kpre[lane + 1] - gs.kpre[lane], vl = gs.vpre[lane + 1] - gs.vpre[lane];
      P.key_len[gr] = uint16_t(kl);
      P.val_len[gr] = vl;
      P.key_off[gr] = m.B.kb0 + gs.kpre[lane];
      P.val_off[gr] = m.B.vb0 + gs.vpre[lane];
    };
    if (sm.staged[lb]) {
      const Staged src{&sm.stage[lb][0], 16 + uint32_t(m.off & 15)};
      build_row_table(src, gs, nr, rec);
      row_index();
      gather_region<false>(src, gs, nr, P.key_arena, m.B.kb0, 0, 1);
      gather_region<true>(src, gs, nr, P.val_arena, m.B.vb0, 0, 1);
    } else {
      const GlobalWin src{P.seg, P.seg_bytes, m.off};
      build_row_table(src, gs, nr, rec);
      row_index();
      gather_region<false>(src, gs, nr, P.key_arena, m.B.kb0, 0, 1);
      gather_region<true>(src, gs, nr, P.val_arena, m.B.vb0, 0, 1);
    }
  }
}



