// okv_decode_ablate.inc -- measured alternatives to pass 3 (DESIGN.md §4.1),
// compiled into libokv_sst_ablate.so only (okv_decode.hip includes this file
// under -DOKV_ABLATE): the per-block global-window gather, the round-2 row
// pass + value sweep, the wave-staged per-block gather, and the source-tile
// pass's measured forms (tile sizes, widths, phase probes, no-DMA / no-store /
// per-chunk / direct-load / sector forms, omitted output classes), each a
// composition of the product's phases (okv_decode.hip, tile_pass) and the
// phases it alters.  The product library (libokv_sst.so) contains none of them.

// The value sweep runs when every row's index is written by the per-block
// pass 3 and the value arena is gap-free: no big block (okv_copy_kernel's
// rows) and no capacity failure.  Every workgroup of both kernels reads the
// same scalars, so they agree.
constexpr uint32_t kSwTile = 4096;  // value-arena bytes per sweep tile
__device__ __forceinline__ bool sweep_safe(const Totals& T, uint32_t nbig, uint64_t row_cap,
                                           uint64_t key_cap, uint64_t val_cap) {
  return nbig == 0 && T.rows <= row_cap && T.kb <= key_cap && T.vb <= val_cap;
}

// Value-sweep hand-off (lane r = row r): each row's value source, the row
// owning each value-arena tile that starts inside its value, and the row's
// boundary chunk.  A 16-byte chunk holding the end of row r's value (end not
// 16-aligned) mixes rows (or the block's zero padding); the lane of the row
// owning its first byte assembles it from the block's row table into
// bchunk[row], and the sweep stores it with its tile (whole lines).  The
// loads are issued first (with the key loads in flight: see okv_rows_kernel).
__device__ __forceinline__ uint4 boundary_chunk(const CopyParams& P, const GatherSmem& sm,
                                                const BlockMeta& m, int rows) {
  const uint32_t t = threadIdx.x;
  uint4 out = make_uint4(0, 0, 0, 0);
  if (int(t) >= rows) return out;
  const uint32_t v0 = sm.vpre[t], e = sm.vpre[t + 1];
  const uint32_t C = e & ~15u;
  if (e == v0 || (e & 15) == 0 || v0 > C) return out;  // no chunk of mine to assemble
  out = merge_bytes(out, window16(P.seg, P.seg_bytes, int64_t(m.off + sm.vsb[t] + C)), 0,
                    int32_t(e - C));
  for (uint32_t j = t + 1; int(j) < rows && sm.vpre[j] < C + 16; ++j) {
    const uint32_t q0 = sm.vpre[j], q1 = sm.vpre[j + 1];
    if (q1 == q0) continue;
    const uint4 w = window16(P.seg, P.seg_bytes, int64_t(m.off + sm.vsb[j] + C));
    out = merge_bytes(out, w, int32_t(q0 - C), int32_t(min(q1, C + 16) - C));
  }
  return out;
}
__device__ __forceinline__ void sweep_handoff(const CopyParams& P, const GatherSmem& sm,
                                              const BlockMeta& m, int rows, const uint4& bc) {
  const uint32_t t = threadIdx.x;
  if (int(t) >= rows) return;
  const uint64_t g = m.B.row0 + t;
  const uint32_t kl = sm.kpre[t + 1] - sm.kpre[t];
  const uint32_t v0 = sm.vpre[t], e = sm.vpre[t + 1];
  P.vsrc[g] = m.off + sm.rec[t] + 6 + kl;
  P.bchunk[g] = bc;
  for (uint64_t x = (m.B.vb0 + v0 + kSwTile - 1) & ~uint64_t(kSwTile - 1); x < m.B.vb0 + e;
       x += kSwTile)
    P.vtile[x / kSwTile] = uint32_t(g);
}

// Pass 3: one workgroup per block reads the block straight from HBM.  NT = 64
// (one wave per block) for small blocks, where a block has only a few 1 KiB
// tiles and more blocks in flight hide the row-table -> gather latency chain;
// NT = 256 otherwise.  The row table's header reads also pull the record
// boundary lines on chip just before the key and value passes need them.
template <int NT>
__global__ __launch_bounds__(NT) void okv_gather_kernel(CopyParams P) {
  __shared__ GatherSmem sm;
  for (uint32_t b = blockIdx.x; b < P.nblk; b += gridDim.x) {
    const BlockMeta m = block_meta(P, b);
    if (block_head(P, b, m)) {
      const int rows = int(m.c.rows);
      const GlobalWin src{P.seg, P.seg_bytes, m.off};
      if (threadIdx.x < 64) {
        const uint32_t t = threadIdx.x;
        const uint32_t rec = int(t) < rows ? P.rt_pos[rec_index(P.nblk, b, t)] : 0u;
        build_row_table(src, sm, rows, rec);
      }
      __syncthreads();
      write_row_index(P, sm, m, rows);
      if (!P.index_only) {
        gather_region<false>(src, sm, rows, P.key_arena, m.B.kb0, threadIdx.x >> 6, NT / 64);
        gather_region<true>(src, sm, rows, P.val_arena, m.B.vb0, threadIdx.x >> 6, NT / 64);
      }
    }
    if (b + gridDim.x < P.nblk) __syncthreads();  // row table reused
  }
}

// Pass 3a of the value sweep: one wave per block writes the row index and
// the key region and hands the values to okv_value_sweep_kernel.  A latency
// chain (metadata -> record positions -> headers -> keys), so it is sized for
// occupancy: one window per lane in flight.  When the sweep is unsafe (big
// blocks, capacity) it gathers the values itself.
__global__ __launch_bounds__(64) void okv_rows_kernel(CopyParams P) {
  __shared__ GatherSmem sm;
  // unsafe for the sweep (big blocks, capacity): okv_gather_staged_kernel,
  // launched after the sweep, does the whole pass instead
  if (!sweep_safe(*P.tot, *P.big_count, P.row_cap, P.key_cap, P.val_cap)) return;
  for (uint32_t b = blockIdx.x; b < P.nblk; b += gridDim.x) {
    // record positions and headers with the metadata (one trip; the slots
    // exist for every block, only the first `rows` are meaningful)
    const uint32_t t = threadIdx.x;
    const uint32_t rec = P.rt_pos[rec_index(P.nblk, b, t)];
    const uint32_t kl = P.rt_kl ? P.rt_kl[rec_index(P.nblk, b, t)] : 0u;
    const BlockMeta m = block_meta(P, b);
    if (block_head(P, b, m)) {
      const int rows = int(m.c.rows);
      const GlobalWin src{P.seg, P.seg_bytes, m.off};
      if (P.rt_kl) {
        // value length from the next record's position (the walk's end after the last)
        const bool live = int(t) < rows;
        uint32_t nxt = __shfl_down(rec, 1, 64);
        if (int(t) == rows - 1) nxt = uint32_t(m.c.pend);
        fill_row_table(sm, rows, live ? rec : 0u, live ? kl : 0u,
                       live ? nxt - rec - 6 - kl : 0u);
      } else {
        build_row_table(src, sm, rows, int(t) < rows ? rec : 0u);
      }
      __syncthreads();
      write_row_index(P, sm, m, rows);
      const uint4 bc = boundary_chunk(P, sm, m, rows);
      gather_tiles<false, GlobalWin, 1>(src, sm, rows, P.key_arena, m.B.kb0, 0,
                                        (sm.kpre[rows] + 1023) >> 10, 1);
      sweep_handoff(P, sm, m, rows, bc);
    }
    if (b + gridDim.x < P.nblk) __syncthreads();  // row table reused
  }
}

// ---------------------------------------------------------------------------
// Pass 3, wave-staged form (experimental, OKV_GATHER_STAGED=1): the value
// region's tiles are produced from a per-wave LDS image of the iteration's
// source span, filled by LDS-DMA (global_load_lds_dwordx4, no VGPR landing):
// the loads in flight no longer cost registers, and a chunk's spill windows
// come from the same image (no second trip).  Keys keep the global windows.
// ---------------------------------------------------------------------------
constexpr uint32_t kStU = 5;                        // value tiles (1 KiB) per iteration
template <uint32_t U> struct StCfg { static constexpr uint32_t cap = U * 1024 + 1024; };

// Row holding region byte x (wave-uniform search over the LDS prefix).
__device__ __forceinline__ uint32_t row_of(const uint32_t* pre, uint32_t last, uint32_t x) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t st = 32; st; st >>= 1) {
    const uint32_t j = pos + st;
    if (j <= last && pre[j] <= x) pos = j;
  }
  return pos;
}

// Tile t of a value region through global windows, for the rare tile whose
// source span does not fit the stage (kept out of line: its registers would
// otherwise size the whole kernel).
__device__ __attribute__((noinline)) void gather_value_tile_global(const uint8_t* seg,
                                                                   uint64_t seg_bytes,
                                                                   uint64_t off,
                                                                   const GatherSmem* sm, int rows,
                                                                   uint8_t* arena, uint64_t dbase,
                                                                   uint32_t t) {
  const GlobalWin src{seg, seg_bytes, off};
  gather_tiles<true, GlobalWin, 1>(src, *sm, rows, arena, dbase, t, t + 1, 1);
}

template <uint32_t U = kStU>
__device__ __forceinline__ bool stage_span(const uint32_t* pre, const uint32_t* sb, uint32_t last,
                                           int64_t off, uint32_t cbeg, uint32_t cend,
                                           int64_t& A, int64_t& E, uint32_t& np) {
  const uint32_t rb = row_of(pre, last, cbeg * 16), re = row_of(pre, last, cend * 16 - 1);
  const int64_t s0 = off + int64_t(sb[rb]) + int64_t(cbeg) * 16;
  const int64_t s1 = off + int64_t(sb[re]) + int64_t(cend) * 16;
  A = (s0 & ~int64_t(15)) - 16;
  E = ((s1 + 15) & ~int64_t(15)) + 16;
  np = uint32_t((E - A + 1023) >> 10);
  return A >= 0 && E - A <= int64_t(StCfg<U>::cap);
}

template <uint32_t kStU>
__device__ __forceinline__ void gather_values_staged(const GlobalWin& src, const GatherSmem& sm,
                                                     int rows, uint8_t* __restrict__ arena,
                                                     uint64_t dbase, uint32_t t0, uint32_t t1,
                                                     uint4* stage) {
  const uint32_t* pre = sm.vpre;
  const uint32_t* sb = sm.vsb;
  const uint32_t N = (pre[rows] + 15) >> 4;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t last = uint32_t(rows) - 1;
  const uint32_t climit = N < t1 * 64 ? N : t1 * 64;  // one past the wave's last chunk
  const int64_t off = int64_t(src.off);
  const uint64_t lim = round16(src.seg_bytes);
  uint32_t r = 0;
  bool searched = false;
  for (uint32_t t = t0; t * 64 < climit;) {
    // kStU tiles per iteration; a span too wide for the stage retries one
    // tile, and a single tile too wide goes through global windows
    uint32_t n = min(kStU, t1 - t);
    uint32_t cbeg = t * 64, cend = min(climit, (t + n) * 64);
    int64_t A, E;
    uint32_t np;
    bool ok = stage_span<kStU>(pre, sb, last, off, cbeg, cend, A, E, np);
    if (!ok && n > 1) {
      n = 1;
      cend = min(climit, (t + 1) * 64);
      ok = stage_span<kStU>(pre, sb, last, off, cbeg, cend, A, E, np);
    }
    if (!ok) {
      gather_value_tile_global(src.seg, src.seg_bytes, src.off, &sm, rows, arena, dbase, t);
      searched = false;
      t += 1;
      continue;
    }
    const uint64_t Eu = uint64_t(E) < lim ? uint64_t(E) : lim;
    for (uint32_t p = 0; p < np; ++p) {
      uint64_t a = uint64_t(A) + (uint64_t(p) << 10) + (lane << 4);
      if (a + 16 > Eu) a = uint64_t(A);  // past the span or the segment: bytes never used
      __builtin_amdgcn_global_load_lds(src.seg + a, OKV_LDS_PTR(stage + p * 64), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (uint32_t u = 0; u < kStU; ++u) {
      if (u >= n) break;
      const uint32_t c = cbeg + u * 64 + lane;
      const bool okc = c < cend;
      const uint32_t x = (okc ? c : cend - 1) << 4, xe = x + 16;
      if (!searched) {
        r = row_of(pre, last, x);
        searched = true;
      } else {
        while (r < last && pre[r + 1] <= x) ++r;
      }
      uint4 out = load16_lds_b128(stage, uint32_t(off + int64_t(sb[r]) + int64_t(x) - A));
      if (okc) {
        if (xe > pre[r + 1]) {
          out = merge_bytes(make_uint4(0, 0, 0, 0), out, 0, int32_t(pre[r + 1] - x));
          for (uint32_t j = r + 1; j <= last && pre[j] < xe; ++j) {
            const uint32_t q0 = pre[j], q1 = pre[j + 1];
            if (q1 == q0) continue;
            const uint4 w =
                load16_lds_b128(stage, uint32_t(off + int64_t(sb[j]) + int64_t(x) - A));
            out = merge_bytes(out, w, int32_t(q0 - x), int32_t((q1 < xe ? q1 : xe) - x));
          }
        }
        *reinterpret_cast<uint4*>(arena + dbase + uint64_t(x)) = out;
      }
    }
    t += n;
  }
}

template <int NT, uint32_t U = kStU>
__global__ __launch_bounds__(NT) void okv_gather_staged_kernel(CopyParams P) {
  __shared__ GatherSmem sm;
  __shared__ uint4 stage[NT / 64][StCfg<U>::cap / 16 + 2];
  // after the value sweep (P.vsrc set): only when the sweep was unsafe
  if (P.vsrc && sweep_safe(*P.tot, *P.big_count, P.row_cap, P.key_cap, P.val_cap)) return;
  for (uint32_t b = blockIdx.x; b < P.nblk; b += gridDim.x) {
    const BlockMeta m = block_meta(P, b);
    if (block_head(P, b, m)) {
      const int rows = int(m.c.rows);
      const GlobalWin src{P.seg, P.seg_bytes, m.off};
      if (threadIdx.x < 64) {
        const uint32_t t = threadIdx.x;
        const uint32_t rec = int(t) < rows ? P.rt_pos[rec_index(P.nblk, b, t)] : 0u;
        build_row_table(src, sm, rows, rec);
      }
      __syncthreads();
      write_row_index(P, sm, m, rows);
      const uint32_t wave = threadIdx.x >> 6;
      const uint32_t Tk = (sm.kpre[rows] + 1023) >> 10;
      gather_tiles<false, GlobalWin, 2>(src, sm, rows, P.key_arena, m.B.kb0,
                                        uint32_t(uint64_t(Tk) * wave / (NT / 64)),
                                        uint32_t(uint64_t(Tk) * (wave + 1) / (NT / 64)), 1);
      const uint32_t T = (sm.vpre[rows] + 1023) >> 10;
      gather_values_staged<U>(src, sm, rows, P.val_arena, m.B.vb0,
                              uint32_t(uint64_t(T) * wave / (NT / 64)),
                              uint32_t(uint64_t(T) * (wave + 1) / (NT / 64)), stage[wave]);
    }
    if (b + gridDim.x < P.nblk) __syncthreads();  // row table reused
  }
}

// ---------------------------------------------------------------------------
// Pass 3b, value sweep: the value arena in address order, one short-lived
// workgroup per kU x 4 KiB of destination (dispatch order = address order, so
// the chip's loads and stores stay in one compact window of source and
// destination -- the one-shot copy shape, DESIGN.md §4).  Lane l of tile t
// produces the 16-byte chunk at X = 4096 t + 16 l: the owning row (the last
// with val_off <= X) comes from the tile's rows [vtile[t], vtile[t + kU]],
// staged in LDS; its bytes from two aligned 16-byte loads + the funnel; bytes
// past its value from the following rows (val_off < X + 16); the rest zero.
// ---------------------------------------------------------------------------
constexpr uint32_t kSwRows = 256;  // rows of a sweep workgroup held in LDS
struct SweepParams {
  const uint8_t* seg;
  uint64_t seg_bytes;
  const uint64_t* val_off;
  const uint32_t* val_len;
  const uint64_t* vsrc;
  const uint32_t* vtile;
  const uint4* bchunk;
  uint8_t* val_arena;
  const Totals* tot;
  const uint32_t* big_count;
  uint64_t row_cap, key_cap, val_cap;
};

// Rows of a sweep workgroup in LDS, relative to its first byte X0: value
// start and end (clamped to +-2^30: only their order against chunk positions
// in [0, kU x 4096) matters) and the source bias (segment position of arena
// byte X = bias + X).
struct SweepRows {
  int32_t rel[kSwRows];
  int32_t end[kSwRows];
  int64_t bias[kSwRows];
};
__device__ __forceinline__ int32_t clamp_rel(int64_t v) {
  return int32_t(v < -(int64_t(1) << 30) ? -(int64_t(1) << 30)
                                         : (v > (int64_t(1) << 30) ? (int64_t(1) << 30) : v));
}

// Workgroups whose rows overflow the LDS window (tiny values): rows past the
// window come from HBM.
__device__ __noinline__ uint4 sweep_chunk_any(const uint8_t* seg, uint64_t seg_bytes,
                                              const uint64_t* val_off, const uint32_t* val_len,
                                              const uint64_t* vsrc, uint64_t r0, uint64_t r1,
                                              uint64_t rows, uint64_t X) {
  uint64_t lo = r0, hi = r1;  // invariant: val_off[lo] <= X
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (val_off[mid] <= X) lo = mid; else hi = mid - 1;
  }
  uint64_t k = lo;
  uint64_t ko = val_off[k];
  uint32_t kl = val_len[k];
  const uint4 w = window16(seg, seg_bytes, int64_t(vsrc[k] + (X - ko)));
  uint4 out = merge_bytes(make_uint4(0, 0, 0, 0), w, 0, int32_t(min<uint64_t>(16, ko + kl - X)));
  for (++k; k < rows; ++k) {
    ko = val_off[k];
    if (ko >= X + 16) break;
    kl = val_len[k];
    if (kl == 0) continue;
    const uint4 v = window16(seg, seg_bytes, int64_t(vsrc[k]) - int64_t(ko - X));
    out = merge_bytes(out, v, int32_t(ko - X), int32_t(min<uint64_t>(16, ko + kl - X)));
  }
  return out;
}

template <uint32_t kU, bool kAl = false>
__global__ __launch_bounds__(256) void okv_value_sweep_kernel(SweepParams S) {
  __shared__ SweepRows R;
  const uint64_t tile0 = uint64_t(blockIdx.x) * kU;
  // one trip for every scalar: the totals, the big-block count and the two
  // tile entries (tile0 + kU <= tiles launched + 1: inside the table)
  const Totals T = *S.tot;
  const uint32_t nbig = *S.big_count;
  const uint32_t e0 = S.vtile[tile0], e1 = S.vtile[tile0 + kU];
  if (!sweep_safe(T, nbig, S.row_cap, S.key_cap, S.val_cap)) return;
  const uint64_t X0 = tile0 * kSwTile;
  if (X0 >= T.vb) return;
  const uint64_t ntile = (T.vb + kSwTile - 1) / kSwTile;
  // rows [r0, r1] cover the workgroup's bytes; r1 + 1 ends the last spill
  // check.  (Clamped into [0, rows): every index stays inside the row arrays
  // whatever the table holds.)
  const uint64_t r0 = min<uint64_t>(e0, T.rows - 1);
  const uint64_t r1 =
      tile0 + kU < ntile ? min<uint64_t>(max<uint64_t>(e1, r0), T.rows - 1) : T.rows - 1;
  const uint64_t rend = min<uint64_t>(r1 + 1, T.rows - 1);
  const bool full = rend - r0 + 1 <= kSwRows;  // uniform
  const uint32_t nw = uint32_t(min<uint64_t>(rend - r0 + 1, kSwRows));
  const uint32_t tid = threadIdx.x;
  if (tid < nw) {
    const int64_t off = int64_t(S.val_off[r0 + tid]);
    const uint32_t len = S.val_len[r0 + tid];
    const int64_t src = int64_t(S.vsrc[r0 + tid]);
    R.rel[tid] = clamp_rel(off - int64_t(X0));
    R.end[tid] = clamp_rel(off + int64_t(len) - int64_t(X0));
    R.bias[tid] = src - off;
  }
  __syncthreads();
  uint4 out[kU];
  bool put[kU];
  uint4 nxt[kU];        // kAl: the next aligned line, where this lane loads it
  uint32_t sft[kU];     // kAl: byte offset of the chunk in its line (0: no funnel)
  bool own[kU];
#pragma unroll
  for (uint32_t u = 0; u < kU; ++u) {
    sft[u] = 0;
    own[u] = false;
    nxt[u] = make_uint4(0, 0, 0, 0);
  }
  // every load issued before any is used
#pragma unroll
  for (uint32_t u = 0; u < kU; ++u) {
    const int32_t xr = int32_t(u * kSwTile + 16u * tid);
    const uint64_t X = X0 + uint32_t(xr);
    out[u] = make_uint4(0, 0, 0, 0);
    put[u] = X < T.vb;
    if (!full || !put[u]) continue;
    // owner: last local row with rel <= xr (rel is non-decreasing)
    uint32_t o = 0;
    if (nw <= 8) {
      for (uint32_t j = 1; j < nw; ++j) o = R.rel[j] <= xr ? j : o;
    } else {
      uint32_t hi = nw - 1;
      while (o < hi) {
        const uint32_t mid = (o + hi + 1) >> 1;
        if (R.rel[mid] <= xr) o = mid; else hi = mid - 1;
      }
    }
    // one unaligned 16-byte load inside the owner's value, or the owner's
    // boundary chunk (okv_rows_kernel).  kAl: the aligned line holding the
    // chunk's first byte; the next line comes from lane + 1 (the next chunk of
    // the same row) by a shuffle, or is loaded here when that lane holds no
    // such chunk (lane 63, the row's last whole chunk)
    const bool whole = xr + 16 <= R.end[o];
    if constexpr (kAl) {
      const int64_t src = R.bias[o] + int64_t(X);
      sft[u] = whole ? uint32_t(src & 15) : 0u;
      own[u] = whole && sft[u] && ((tid & 63) == 63 || xr + 32 > R.end[o]);
      if (whole) {
        const uint4* line = reinterpret_cast<const uint4*>(S.seg + (src & ~int64_t(15)));
        out[u] = line[0];
        if (own[u]) nxt[u] = line[1];
      } else {
        out[u] = S.bchunk[r0 + o];
      }
    } else {
      if (whole)
        out[u] = *reinterpret_cast<const uint4*>(S.seg + (R.bias[o] + int64_t(X)));
      else
        out[u] = S.bchunk[r0 + o];
    }
  }
  if constexpr (kAl) {
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint4 nb = make_uint4(__shfl_down(out[u].x, 1, 64), __shfl_down(out[u].y, 1, 64),
                                  __shfl_down(out[u].z, 1, 64), __shfl_down(out[u].w, 1, 64));
      if (sft[u]) out[u] = funnel32(out[u], own[u] ? nxt[u] : nb, sft[u]);
    }
  }
  if (!full) {
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint64_t X = X0 + uint64_t(u) * kSwTile + 16u * tid;
      if (put[u])
        out[u] = sweep_chunk_any(S.seg, S.seg_bytes, S.val_off, S.val_len, S.vsrc, r0, r1, T.rows,
                                 X);
    }
  }
#pragma unroll
  for (uint32_t u = 0; u < kU; ++u) {
    const uint64_t X = X0 + uint64_t(u) * kSwTile + 16u * tid;
    if (put[u]) *reinterpret_cast<uint4*>(S.val_arena + X) = out[u];
  }
}


// ---------------------------------------------------------------------------
// The source-tile pass's measured forms.  Each is the product's sequence of
// phases (okv_decode.hip, tile_pass) with the phases it alters, which live
// here; the product's phases carry no flag for them.
// ---------------------------------------------------------------------------

// A destination chunk of a tile whose owned bytes [lo, hi) span rows or
// padding: each row's piece from a global window (rare; kept out of line).
__device__ __noinline__ uint4 tile_chunk_pieces(const uint8_t* seg, uint64_t seg_bytes, uint64_t off,
                                                const uint32_t* pre, const uint32_t* sb,
                                                uint32_t rows, uint32_t r, uint32_t x,
                                                uint32_t lo, uint32_t hi) {
  return chunk_bytes(pre, sb, rows, r, x, lo, hi,
                     [&](uint32_t s) { return window16(seg, seg_bytes, int64_t(off + s)); });
}

// The round-5 extent: no stage extension (every form without the line cut).
template <uint32_t kT>
__device__ __forceinline__ TileExtent tile_extent_r5(const TileBlock& B) {
  TileExtent X = tile_extent<kT>(B);
  if (!X.last_tile) X.np -= kLineExt / 16;
  return X;
}

// The per-chunk store (d3-d5, d8): every key and value chunk looked up per
// lane through the two granule tables.  kDiag 4: no stores; 5: no data reads.
template <uint32_t kNT, int kDiag, class Rows>
__device__ __forceinline__ void chunk_store(const CopyParams& P, const TileBlock& B,
                                            const TileExtent& X, const Rows& R,
                                            const uint8_t* gtk, const uint8_t* gtv,
                                            const uint4* stage, const TileOwned& O) {
  const uint32_t nk = O.kx1 > O.kx0 ? ((O.kx1 + 15) >> 4) - (O.kx0 >> 4) : 0u;
  const uint32_t nv = O.vx1 > O.vx0 ? ((O.vx1 + 15) >> 4) - (O.vx0 >> 4) : 0u;
  const uint32_t sbias = uint32_t(int64_t(B.off) - X.A);
  for (uint32_t j = threadIdx.x; j < nk + nv; j += kNT) {
    const uint32_t reg = j >= nk;
    const uint32_t X0 = reg ? O.vx0 : O.kx0, X1 = reg ? O.vx1 : O.kx1;
    const uint32_t x = ((X0 >> 4) + (reg ? j - nk : j)) << 4;
    const uint32_t lo = max(x, X0), hi = min(x + 16, X1);
    const uint32_t* pre = R.pre[reg];
    const uint32_t* sb = R.sb[reg];
    uint32_t r = (reg ? gtv : gtk)[(lo >> 6) - (X0 >> 6)];
    while (r < X.lastr && pre[r + 1] <= lo) ++r;
    uint8_t* dst = (reg ? P.val_arena + B.vb0 : P.key_arena + B.kb0) + x;
    if (lo == x && hi == x + 16 && pre[r + 1] >= x + 16) {  // the common chunk: inside row r
      if constexpr (kDiag == 5) {  // diagnostic: the lookup, no data read
        *reinterpret_cast<uint4*>(dst) = make_uint4(r, x, 0, 0);
        continue;
      }
      const uint4 w = load16_lds_b128(stage, sb[r] + x + sbias);
      if constexpr (kDiag == 4) {  // diagnostic: no stores
        asm volatile("" ::"v"(w.x), "v"(w.y), "v"(w.z), "v"(w.w));
        continue;
      }
      *reinterpret_cast<uint4*>(dst) = w;
      continue;
    }
    const uint4 out = chunk_bytes(pre, sb, X.rows, r, x, lo, hi, [&](uint32_t s) {
      return load16_lds_b128(stage, s + sbias);
    });
    if (lo == x && hi == x + 16)
      *reinterpret_cast<uint4*>(dst) = out;
    else
      store_partial(dst, out, lo - x, hi - x);
  }
}

// The direct store (d6): no LDS stage, one unaligned global load per chunk,
// every load issued before any store.
template <uint32_t kT, uint32_t kNT, class Rows>
__device__ __forceinline__ void direct_store(const CopyParams& P, const TileBlock& B,
                                             const TileExtent& X, const Rows& R,
                                             const uint8_t* gtk, const uint8_t* gtv,
                                             const TileOwned& O) {
  constexpr uint32_t kU = (kT / 16 + 8 + kNT - 1) / kNT;  // chunk slots per lane
  const uint32_t nk = O.kx1 > O.kx0 ? ((O.kx1 + 15) >> 4) - (O.kx0 >> 4) : 0u;
  const uint32_t nv = O.vx1 > O.vx0 ? ((O.vx1 + 15) >> 4) - (O.vx0 >> 4) : 0u;
  uint4 v[kU];
  uint32_t xs[kU], los[kU], his[kU], regs[kU];
  bool slow[kU];
#pragma unroll
  for (uint32_t u = 0; u < kU; ++u) {
    const uint32_t j = threadIdx.x + u * kNT;
    his[u] = 0;
    los[u] = 0;
    slow[u] = false;
    v[u] = make_uint4(0, 0, 0, 0);
    if (j >= nk + nv) continue;
    const uint32_t reg = j >= nk;
    const uint32_t X0 = reg ? O.vx0 : O.kx0, X1 = reg ? O.vx1 : O.kx1;
    const uint32_t x = ((X0 >> 4) + (reg ? j - nk : j)) << 4;
    const uint32_t lo = max(x, X0), hi = min(x + 16, X1);
    const uint32_t* pre = R.pre[reg];
    uint32_t r = (reg ? gtv : gtk)[(lo >> 6) - (X0 >> 6)];
    while (r < X.lastr && pre[r + 1] <= lo) ++r;
    xs[u] = x;
    los[u] = lo;
    his[u] = hi;
    regs[u] = reg | (r << 1);
    if (lo == x && hi == x + 16 && pre[r + 1] >= x + 16)
      v[u] = *reinterpret_cast<const uint4*>(P.seg + B.off + R.sb[reg][r] + x);
    else
      slow[u] = true;
  }
#pragma unroll
  for (uint32_t u = 0; u < kU; ++u)
    if (slow[u])
      v[u] = tile_chunk_pieces(P.seg, P.seg_bytes, B.off, R.pre[regs[u] & 1], R.sb[regs[u] & 1],
                               X.rows, regs[u] >> 1, xs[u], los[u], his[u]);
#pragma unroll
  for (uint32_t u = 0; u < kU; ++u) {
    if (his[u] <= los[u]) continue;
    uint8_t* dst = ((regs[u] & 1) ? P.val_arena + B.vb0 : P.key_arena + B.kb0) + xs[u];
    if (los[u] == xs[u] && his[u] == xs[u] + 16)
      *reinterpret_cast<uint4*>(dst) = v[u];
    else
      store_partial(dst, v[u], los[u] - xs[u], his[u] - xs[u]);
  }
}

// Every cut between two tiles of a block moves up to a 64-byte sector of the
// arena, so no destination sector is shared by two tiles; the few bytes this
// adds to the tile before the cut come from global windows when they lie past
// its stage.  (kKeyRound false: key cuts left as they are.)
template <bool kKeyRound>
__device__ __forceinline__ void sector_cuts(const TileBlock& B, const TileExtent& X, TileCuts& C) {
  auto sector_up = [](uint32_t Y, uint64_t base, uint32_t tot) -> uint32_t {
    const uint32_t end = uint32_t(round16(tot));
    const uint32_t Ys = uint32_t(((base + Y + 63) & ~uint64_t(63)) - base);
    return Ys > end ? end : Ys;
  };
  if (B.t != 0) {
    if (kKeyRound) C.x[0] = sector_up(C.x[0], B.kb0, C.KT);
    C.x[2] = sector_up(C.x[2], B.vb0, C.VT);
  }
  if (!X.last_tile) {
    if (kKeyRound) C.x[1] = sector_up(C.x[1], B.kb0, C.KT);
    C.x[3] = sector_up(C.x[3], B.vb0, C.VT);
  }
  C.x[0] = min(C.x[0], C.x[1]);
  C.x[2] = min(C.x[2], C.x[3]);
}

// Row pieces of the owned value range: [a, e) = row r's bytes in [X2, X3).
// Runs: the whole 64-byte sectors inside a piece (and before Yv1, the
// unrounded value cut at P1: value bytes before it have their sources in this
// tile's stage), in units of <= 64 chunks -- one wave store writes whole
// sectors.  Every other sector a piece touches is a mixed sector: its four
// chunks are assembled by four adjacent lanes and stored by one instruction.
template <class Rows>
__device__ __forceinline__ void sector_value_units(const TileBlock& B, const TileExtent& X,
                                                   const TileLane& W, const TileCuts& C,
                                                   uint32_t Yv1, Rows& R) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t vb0 = B.vb0;
  const uint32_t a = max(W.vp, C.x[2]), e = min(W.vp + W.v, C.x[3]);
  const bool piece = W.live && W.v && a < e;
  const uint64_t va = vb0 + a, ve = vb0 + min(e, Yv1);
  const uint64_t s0 = (va + 63) & ~uint64_t(63), s1 = ve & ~uint64_t(63);
  const bool run = piece && s1 > s0;
  const uint32_t cs = run ? uint32_t((s0 - vb0) >> 4) : 0u;
  const uint32_t wc = run ? uint32_t((s1 - s0) >> 4) : 0u;
  const uint32_t nu = (wc + 63) >> 6;
  const uint32_t ui = wave_scan_dpp(nu);
  const uint32_t sbias0 = uint32_t(int64_t(B.off) - X.A);
  for (uint32_t q = 0; q < nu; ++q) {
    const uint32_t u = ui - nu + q;
    R.unit[0][u] = cs + 64 * q;
    R.unit[1][u] = W.vs - W.vp + 16 * (cs + 64 * q) + sbias0;
    R.unit[2][u] = min(64u, wc - 64 * q);
  }
  // mixed sectors, as (sector - the region's first sector) << 8 | the
  // lowest row with bytes in it (rows in order, head before tail; equal
  // neighbours skipped by the consumer)
  const uint64_t vs0 = vb0 >> 6;
  const uint32_t hsec = uint32_t(((vb0 + a) >> 6) - vs0);
  const uint32_t tsec = uint32_t(((vb0 + e - 1) >> 6) - vs0);
  const bool need_h = piece && (!run || s0 > va);
  const bool need_t = piece && (run ? s1 < vb0 + e : tsec != hsec);
  const uint32_t nme = uint32_t(need_h) + uint32_t(need_t);
  const uint32_t mi = wave_scan_dpp(nme) - nme;
  if (need_h) R.bnd[mi] = (hsec << 8) | lane;
  if (need_t) R.bnd[mi + uint32_t(need_h)] = (tsec << 8) | lane;
  const uint32_t nunit = __builtin_amdgcn_readlane(ui, 63);
  const uint32_t nmix = __builtin_amdgcn_readlane(mi + nme, 63);
  if (lane == 0) {
    R.nbnd = nmix;
    R.nunit = nunit;
  }
}

// Keys (from the first chunk of the range's first sector, so each wave store
// covers whole sectors) and the mixed value sectors, four lanes each: per-lane
// lookup; sources past the stage from global windows.
template <uint32_t kNT, bool kNoKeys, class Rows>
__device__ __forceinline__ void sector_store(const CopyParams& P, const TileBlock& B,
                                             const TileExtent& X, const Rows& R,
                                             const uint8_t* gt, const uint4* stage,
                                             const TileOwned& O) {
  const uint32_t nk = O.kx1 > O.kx0 ? ((O.kx1 + 15) >> 4) - (O.kx0 >> 4) : 0u;
  const uint32_t sbias = uint32_t(int64_t(B.off) - X.A);
  const uint32_t kc0 = O.kx0 >> 4;
  const uint32_t kph = uint32_t(((B.kb0 >> 4) + kc0) & 3u);
  const uint32_t nk4 = nk ? (kph + nk + 3) & ~3u : 0u;
  const uint32_t vph = uint32_t(B.vb0 & 63);
  for (uint32_t j = threadIdx.x; j < nk4 + 4 * O.nbnd; j += kNT) {
    const uint32_t reg = j >= nk4;
    if (kNoKeys && !reg) continue;
    uint32_t r;
    int32_t xs;
    if (reg) {
      const uint32_t ei = (j - nk4) >> 2;
      const uint32_t bv = R.bnd[ei];
      if (ei && (bv >> 8) == (R.bnd[ei - 1] >> 8)) continue;
      xs = int32_t((bv >> 8) * 64u) - int32_t(vph) + int32_t(16 * ((j - nk4) & 3u));
      r = bv & 255u;
    } else {
      xs = int32_t(16 * (kc0 + j)) - int32_t(16 * kph);
      r = 0;
    }
    const uint32_t X0 = reg ? O.vx0 : O.kx0, X1 = reg ? O.vx1 : O.kx1;
    if (xs + 16 <= int32_t(X0) || xs >= int32_t(X1)) continue;
    const uint32_t x = uint32_t(xs);
    const uint32_t lo = max(x, X0), hi = min(x + 16, X1);
    const uint32_t* pre = R.pre[reg];
    const uint32_t* sb = R.sb[reg];
    if (!reg) r = uint32_t(gt[(lo >> 6) - (X0 >> 6)]);
    while (r < X.lastr && pre[r + 1] <= lo) ++r;
    uint8_t* dst = (reg ? P.val_arena + B.vb0 : P.key_arena + B.kb0) + x;
    const uint4 out = chunk_bytes(pre, sb, X.rows, r, x, lo, hi, [&](uint32_t s) {
      return (((s + sbias) >> 4) + 1 < X.np) ? load16_lds_b128(stage, s + sbias)
                                             : window16(P.seg, P.seg_bytes, int64_t(B.off) + s);
    });
    if (lo == x && hi == x + 16)
      *reinterpret_cast<uint4*>(dst) = out;
    else
      store_partial(dst, out, lo - x, hi - x);
  }
}

// The product's key and boundary-chunk store with output classes left out:
// 4 key chunks, 8 boundary value chunks, 16 partial chunks.
template <uint32_t kNT, uint32_t kSkip, class Rows>
__device__ __forceinline__ void skip_store_chunks(const CopyParams& P, const TileBlock& B,
                                                  const TileExtent& X, const Rows& R,
                                                  const uint8_t* gt, const uint4* stage,
                                                  const TileOwned& O) {
  const uint32_t nk = O.kx1 > O.kx0 ? ((O.kx1 + 15) >> 4) - (O.kx0 >> 4) : 0u;
  for (uint32_t j = threadIdx.x; j < nk + O.nbnd; j += kNT) {
    if ((kSkip & 4) && j < nk) continue;
    if ((kSkip & 8) && j >= nk) continue;
    TileChunk c;
    if (!tile_chunk(P, B, X, R, gt, stage, O, nk, j, c)) continue;
    if (c.lo == 0 && c.hi == 16)
      *reinterpret_cast<uint4*>(c.dst) = c.out;
    else if (!(kSkip & 16))
      store_partial(c.dst, c.out, c.lo, c.hi);
  }
}

// Every form but d0 and d9 (the product's tile_pass): the product's sequence
// with the phases the form alters.
// Forms d32 + kSkip -- output classes left unwritten, to attribute the pass's
// HBM write traffic: 1 the SoA row index, 2 value runs, 4 key chunks, 8
// boundary value chunks, 16 partial chunks; other cuts: 64 the round-5 cuts
// (no line cut, no stage extension); 128 whole 64-byte sectors per store
// (+ 256 key cuts unrounded, + 512 the stage extension).  d32 is the product's
// sequence.
// Forms d1-d8, all on the round-5 cuts: 1 no chunk pass, 2 no DMA, 3 phase
// probe of the per-chunk form, 4 (+ no stores), 5 (+ no data reads), 6 direct
// unaligned global loads, 7 phase probe of the value-run form, 8 the per-chunk
// form (every chunk looked up per lane).
template <uint32_t kT, uint32_t kNT, bool kXcd, uint32_t kDiag>
__device__ __forceinline__ void tile_pass_diag(const CopyParams& P, uint32_t tpb, uint32_t ntile) {
  constexpr uint32_t kSkip = kDiag >= 32 ? kDiag - 32 : 64u;
  constexpr bool kDirect = kDiag == 6;  // no LDS stage
  constexpr bool kChunk = (kDiag >= 3 && kDiag <= 5) || kDiag == 8;
  constexpr bool kRuns = !kChunk && !kDirect;
  constexpr bool kProbe = (kDiag >= 3 && kDiag <= 5) || kDiag == 7;
  constexpr bool kSector = (kSkip & 128) != 0;
  constexpr bool kLineCut = !(kSkip & 64) && !kSector;
  constexpr bool kExt = kLineCut || (kSkip & 512);
  __shared__ TileRows<kT> R;
  __shared__ uint8_t gt[kRuns ? 1 : 2][kT / 64 + 8];  // [key, value] granule tables
  __shared__ uint4 stage[(kT + (kExt ? kLineExt : 0)) / 16 + 4];
  const uint32_t L = tile_index<kXcd>();
  if (L >= ntile) return;
  uint64_t T[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // kProbe: phase timestamps
  if constexpr (kProbe) T[0] = __builtin_amdgcn_s_memrealtime();
  uint32_t rec, kl;
  const TileBlock B = tile_block(P, L, tpb, rec, kl);
  if constexpr (kProbe) T[1] = __builtin_amdgcn_s_memrealtime();
  if (tile_idle<kT>(P, B)) {
    block_outputs(P, B);
    return;
  }
  const TileExtent X = kExt ? tile_extent<kT>(B) : tile_extent_r5<kT>(B);
  if constexpr (kDiag != 2 && !kDirect) tile_dma<kNT>(P, B, X, stage);
  if constexpr (kProbe) T[2] = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x < 64) {
    const TileLane W = tile_row_table(B, X, rec, kl, R);
    if (!P.index_only) {
      TileCuts C = tile_owned_ranges(W, X);
      if constexpr (kLineCut) tile_line_cut(B, X, W, C);
      const uint32_t Yv1 = C.x[3];
      if constexpr (kSector) sector_cuts<!(kSkip & 256)>(B, X, C);
      tile_put_cuts(C, R);
      tile_granules(X, W.live, W.kp, W.k, C.x[0], C.x[1], gt[0]);
      // the value-run forms need the key table only (a 4 KiB value is 64
      // granules, a serial per-lane loop)
      if constexpr (kSector)
        sector_value_units(B, X, W, C, Yv1, R);
      else if constexpr (kRuns)
        tile_value_units(B, X, W, C, R);
      else
        tile_granules(X, W.live, W.vp, W.v, C.x[2], C.x[3], gt[1]);
    }
    tile_index_rows(P, B, W);
  }
  if constexpr (kProbe) T[3] = __builtin_amdgcn_s_memrealtime();
  if (P.index_only) {
    block_outputs(P, B);
    return;
  }
  tile_wait_stage();
  if constexpr (kProbe) T[4] = __builtin_amdgcn_s_memrealtime();
  if constexpr ((kSkip & 1) != 0)
    block_outputs(P, B);
  else
    tile_row_index(P, B, X, R);
  if (kDiag == 1) return;  // diagnostic: metadata + DMA + row table only
  const TileOwned O = tile_owned(R);
  if constexpr (kRuns && !(kSkip & 2)) tile_store_runs<kNT>(P, B, R, stage, O.nunit);
  if constexpr (kSector)
    sector_store<kNT, (kSkip & 4) != 0>(P, B, X, R, gt[0], stage, O);
  else if constexpr (kRuns)
    skip_store_chunks<kNT, kSkip>(P, B, X, R, gt[0], stage, O);
  else if constexpr (kDirect)
    direct_store<kT, kNT>(P, B, X, R, gt[0], gt[1], O);
  else
    chunk_store<kNT, kDiag>(P, B, X, R, gt[0], gt[1], stage, O);
  if constexpr (kProbe) {  // the last three timestamps; sampled workgroups hand theirs over
    T[5] = __builtin_amdgcn_s_memrealtime();
    __syncthreads();
    T[6] = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    T[7] = __builtin_amdgcn_s_memrealtime();
    if ((L & 255) == 0 && threadIdx.x == 0)
      for (int k = 0; k < 8; ++k) P.vsrc[(L >> 8) * 8 + k] = T[k];
  }
}

// 8 waves per SIMD as the product.
template <uint32_t kT, uint32_t kNT, bool kXcd, uint32_t kDiag>
__global__ __launch_bounds__(kNT) __attribute__((amdgpu_waves_per_eu(kT <= 16384 || kNT == 1024 ? 8 : 4))) void okv_tile_kernel_diag(
    CopyParams P, uint32_t tpb, uint32_t ntile) {
  tile_pass_diag<kT, kNT, kXcd, kDiag>(P, tpb, ntile);
}
template <uint32_t kT, uint32_t kNT, bool kXcd, uint32_t kSkip>
__global__ __launch_bounds__(kNT) __attribute__((amdgpu_waves_per_eu(8))) void okv_tile_kernel_skip(
    CopyParams P, uint32_t tpb, uint32_t ntile) {
  tile_pass_diag<kT, kNT, kXcd, kSkip + 32>(P, tpb, ntile);
}
// Form d9: the product's tile_pass without the 8-waves register cap.
template <uint32_t kT, uint32_t kNT, bool kXcd>
__global__ __launch_bounds__(kNT) void okv_tile_kernel_w7(CopyParams P, uint32_t tpb,
                                                          uint32_t ntile) {
  tile_pass<kT, kNT, kXcd>(P, tpb, ntile);
}
