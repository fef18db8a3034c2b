// Ablation build only (#included by okv_decode.hip under -DOKV_ABLATE): the
// host side of the decode forms that measured slower than the product ones
// and of the diagnostic ones -- their knobs (ablate_open), their scratch,
// their launches and the dispatcher that selects among them (ablate_decode).
// okv_decode.hip enters through one-line hooks: ablate_open, ablate_close,
// ablate_decode, ablate_launch_tile, ablate_count_prefetch (DESIGN.md 13.7.1).

// OKV_DECODE_PIECES=1: large-block decodes in two pieces.  The header walk of
// the first kPieceDiv-th of the blocks, then the tile pass over them on the
// context's stream while the second piece's walk runs on a second stream; the
// second tile pass waits for that walk.  Measured at C3 (r4b, 3 alternating
// runs): count+scan 0.061 vs 0.105 ms but the two tile launches 1.487 vs
// 1.384 ms, step 1.55 vs 1.48 ms: the walk is latency-bound (a dependent chain
// per block, ~0.09 ms at C3 whatever the block count), so the first piece's
// walk costs what the whole walk does, and the second launch adds a tail.
constexpr uint32_t kPieceDiv = 8;
constexpr uint32_t kPieceMinBlocks = 8192;
uint32_t piece_split(uint32_t nblk) {
  if (nblk < kPieceMinBlocks) return 0;
  return (nblk / kPieceDiv) & ~uint32_t(kTile - 1);  // a multiple of the count kernel's tile
}

int ensure_pieces(okv_ctx* ctx) {
  if (ctx->ab.stream2) return OKV_OK;
  OKV_HIP(hipStreamCreateWithFlags(&ctx->ab.stream2, hipStreamNonBlocking));
  OKV_HIP(hipEventCreateWithFlags(&ctx->ab.ev_piece[0], hipEventDisableTiming));
  OKV_HIP(hipEventCreateWithFlags(&ctx->ab.ev_piece[1], hipEventDisableTiming));
  return reserve(ctx, ctx->ab.d_tot2, 1);
}

// Pass 1-2 of blocks [b0, b0 + n) (b0 a multiple of kTile) on stream s,
// continuing the prefixes of the blocks before them (base: their totals, or
// null), totals into tot; the piece's record tables at b0 * kRCap (its own
// layout).  The first piece's launch zeroes the other big-block counter slot.
void launch_count_piece(okv_ctx* ctx, hipStream_t s, const Work& w, uint32_t b0, uint32_t n,
                        uint64_t* d_row_start, const Totals* base, Totals* tot, bool first,
                        uint16_t* rt_kl = nullptr, uint64_t span_cap = ~0ull) {
  const uint64_t t0 = b0 / kTile;
  hipLaunchKernelGGL(okv_count_kernel, dim3((n + kTile - 1) / kTile), dim3(kThreads), 0, s, w.seg,
                     w.seg_bytes, w.descs + b0, n, w.comp, ctx->d_cnt.data() + b0,
                     ctx->d_lp.data() + b0, ctx->d_tile_tot.data() + t0,
                     ctx->d_rec.data() + uint64_t(b0) * kRCap,
                     rt_kl ? rt_kl + uint64_t(b0) * kRCap : nullptr, ctx->d_big.data(),
                     big_counter(ctx), w.pre ? w.pre + b0 : nullptr, 0, span_cap,
                     ctx->d_tile_pre.data() + t0, tot, d_row_start ? d_row_start + b0 : nullptr,
                     ctx->d_ctr.data() + kCtrArrive, first ? big_counter(ctx, 1) : nullptr, base,
                     b0, nullptr);
}

// Passes 1-2 as two launches: blocks [0, b0) on the context stream (totals
// into d_tot2), then -- once they are done -- blocks [b0, nblk) on stream2,
// their prefixes continuing from d_tot2 (final totals into d_tot).
int launch_plan_pieces(okv_ctx* ctx, const Work& w, uint32_t nblk, uint32_t b0,
                       uint64_t* d_row_start, uint16_t* rt_kl, uint64_t span_cap) {
  AblateState& A = ctx->ab;
  int rc = ensure_pieces(ctx);
  if (rc) return rc;
  launch_count_piece(ctx, ctx->stream, w, 0, b0, nullptr, nullptr, A.d_tot2.data(), true, rt_kl,
                     span_cap);
  OKV_HIP(hipGetLastError());
  OKV_HIP(hipEventRecord(A.ev_piece[0], ctx->stream));
  OKV_HIP(hipStreamWaitEvent(A.stream2, A.ev_piece[0], 0));
  launch_count_piece(ctx, A.stream2, w, b0, nblk - b0, d_row_start, A.d_tot2.data(),
                     ctx->d_tot.data(), false, rt_kl, span_cap);
  OKV_HIP(hipGetLastError());
  OKV_HIP(hipEventRecord(A.ev_piece[1], A.stream2));
  ctx->big_slot ^= 1u;  // the first launch zeroed the other slot
  prof_mark(ctx, 2);
  prof_mark(ctx, 3);
  return OKV_OK;
}

// The CopyParams of blocks [b0, b0 + n) of P (block-indexed arrays advanced;
// row and arena positions stay global).
CopyParams piece_params(const CopyParams& P, uint32_t b0, uint32_t n) {
  CopyParams Q = P;
  Q.descs = P.descs + b0;
  Q.nblk = n;
  Q.cnt = P.cnt + b0;
  Q.lp = P.lp + b0;
  Q.tile_pre = P.tile_pre + b0 / kTile;
  Q.rt_pos = P.rt_pos + uint64_t(b0) * kRCap;
  Q.rt_kl = P.rt_kl ? P.rt_kl + uint64_t(b0) * kRCap : nullptr;
  Q.row_start = P.row_start + b0;
  Q.key_base = P.key_base ? P.key_base + b0 : nullptr;
  Q.val_base = P.val_base ? P.val_base + b0 : nullptr;
  Q.blk_status = P.blk_status + b0;
  return Q;
}

// Phase stamps of okv_point_kernel's last block (wall clock, 100 MHz ticks):
// out[0..4] = start, staged, walked, prefixes, emitted.
extern "C" int okv_debug_point_times(uint64_t* out) {
  const size_t n = 5 * sizeof(uint64_t);
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(okv::g_point_t), n) == hipSuccess ? 0 : -1;
}

// Phase stamps of okv_decode_fused_kernel per block (wall clock, 100 MHz
// ticks): out[b * 8 + 0..4] = start, staged, walked, prefix known, done.
extern "C" int okv_debug_fused_times(uint64_t* out, uint32_t nblk) {
  const size_t n = std::min<size_t>(nblk, okv::kFusedMaxBlocks) * 8 * sizeof(uint64_t);
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(okv::g_fused_t), n) == hipSuccess ? 0 : -1;
}

// Look-back scratch of the grouped single pass (one 4-byte flag per group).
int ensure_group(okv_ctx* ctx, uint32_t ngroups) {
  AblateState& A = ctx->ab;
  return ensure_lookback(ctx, ngroups, A.g_flag, A.g_agg, A.g_incl);
}

// ---- the tile pass's forms (OKV_TILE=<KiB>[x][w<threads>][d<diag>]) ---------
template <uint32_t kT, uint32_t kNT, bool kXcd, int kDiag>
void launch_tile_t(hipStream_t s, const CopyParams& P, uint32_t tpb, uint32_t ntile) {
  const uint32_t grid = kXcd ? ((ntile + 7u) & ~7u) : ntile;
  if constexpr (kDiag == 0) {  // the product's kernel, at this geometry
    hipLaunchKernelGGL((okv_tile_kernel<kT, kNT, kXcd>), dim3(grid), dim3(kNT), 0, s, P, tpb,
                       ntile);
  } else if constexpr (kDiag == 9) {  // the same without the register cap
    hipLaunchKernelGGL((okv_tile_kernel_w7<kT, kNT, kXcd>), dim3(grid), dim3(kNT), 0, s, P, tpb,
                       ntile);
  } else if constexpr (kDiag >= 32) {
    hipLaunchKernelGGL((okv_tile_kernel_skip<kT, kNT, kXcd, uint32_t(kDiag - 32)>), dim3(grid),
                       dim3(kNT), 0, s, P, tpb, ntile);
  } else {
    hipLaunchKernelGGL((okv_tile_kernel_diag<kT, kNT, kXcd, kDiag>), dim3(grid), dim3(kNT), 0, s,
                       P, tpb, ntile);
  }
}
typedef void (*TileLaunch)(hipStream_t, const CopyParams&, uint32_t, uint32_t);
struct TileForm {
  uint32_t kib, threads, diag;
  TileLaunch x, plain;
};
#define OKV_TILE_FORM(K, N, D)                                                              \
  TileForm {                                                                                \
    K, N, D, launch_tile_t<K * 1024, N, true, D>, launch_tile_t<K * 1024, N, false, D>      \
  }
#define F(K, N, D) OKV_TILE_FORM(K, N, D)
const TileForm kTileForms[] = {
    F(16, 256, 0), F(8, 256, 0), F(32, 256, 0), F(16, 512, 0), F(32, 512, 0), F(4, 256, 0),
    F(16, 256, 1), F(16, 256, 2), F(16, 256, 3), F(16, 256, 4), F(16, 256, 5), F(16, 256, 6),
    F(16, 256, 7), F(16, 256, 8), F(8, 256, 8), F(32, 512, 8), F(16, 256, 9), F(64, 1024, 0),
    F(64, 512, 0),
    // write attribution (okv_tile_kernel_skip): d32 + kSkip
    F(16, 256, 32), F(16, 256, 33), F(16, 256, 34), F(16, 256, 36), F(16, 256, 40),
    F(16, 256, 48), F(16, 256, 63),
    // the round-5 cuts, no line cut (tile_pass_skip kSkip 64); whole 64-byte sectors per store (128)
    F(16, 256, 96), F(16, 256, 160), F(16, 256, 672), F(16, 256, 928)};
#undef F
const TileForm* tile_form(uint32_t kib, uint32_t threads, uint32_t diag) {
  for (const TileForm& f : kTileForms)
    if (f.kib == kib && f.threads == threads && f.diag == diag) return &f;
  return nullptr;
}

// launch_tile's hook: the form the knobs name (ablate_open has checked that it
// exists); with none set, the product form (okv_tile_kernel at the product's geometry).
void ablate_launch_tile(okv_ctx* ctx, const CopyParams& P, const TileGeo& g) {
  const AblateState& A = ctx->ab;
  const TileForm* f = tile_form(A.tile_kib, A.tile_threads, A.tile_diag);
  (A.tile_xcd ? f->x : f->plain)(ctx->stream, P, g.tpb, P.nblk * g.tpb);
}

// launch_plan's hook (OKV_COUNT_PREFETCH=0|1: the count kernel's line prefetch).
int ablate_count_prefetch(int prefetch, uint32_t nblk) {
  const char* v = getenv("OKV_COUNT_PREFETCH");
  return v ? atoi(v) && nblk : prefetch;
}

// okv_open's hook: the knobs of the measured alternative forms
// (tools/ablate*.py), all bit-exact with the product.  Returns ctx, or deletes
// it and returns null when a knob names a form that does not exist.
okv_ctx* ablate_open(okv_ctx* ctx) {
  AblateState& A = ctx->ab;
  auto bad = [&]() -> okv_ctx* {
    delete ctx;
    return nullptr;
  };
  // pass-3 launch: OKV_GATHER_THREADS=64|256 (workgroup width),
  // OKV_GATHER_GRID=<workgroups> (persistent grid)
  if (const char* v = getenv("OKV_GATHER_THREADS")) {
    A.gather_threads = uint32_t(atoi(v));
    if (A.gather_threads != 64 && A.gather_threads != 256) return bad();
  }
  if (const char* v = getenv("OKV_GATHER_GRID")) A.gather_grid = uint32_t(atoi(v));
  if (const char* v = getenv("OKV_DECODE_FUSED")) ctx->fused = atoi(v) != 0;
  if (const char* v = getenv("OKV_DECODE_GROUP")) A.group = atoi(v) != 0;
  if (const char* v = getenv("OKV_DECODE_PIECES")) A.pieces = atoi(v) != 0;
  if (const char* v = getenv("OKV_DECODE_STREAM")) A.stream_lb = atoi(v) != 0;
  if (const char* v = getenv("OKV_SMALL_PIECE_MB")) A.small_piece = uint64_t(atoi(v)) << 20;
  if (const char* v = getenv("OKV_GATHER_STAGED")) A.gather_staged = atoi(v) != 0;
  if (const char* v = getenv("OKV_VALUE_SWEEP")) {
    A.value_sweep = uint32_t(atoi(v));
    if (A.value_sweep > 11 || A.value_sweep == 3) return bad();
  }
  if (const char* v = getenv("OKV_TILE")) {  // <KiB>[x][w<threads>][d<diag>]
    A.tile_kib = uint32_t(atoi(v));
    A.tile_xcd = strchr(v, 'x') != nullptr;
    const char* w = strchr(v, 'w');
    A.tile_threads = w ? uint32_t(atoi(w + 1)) : 256u;
    const char* dg = strchr(v, 'd');
    A.tile_diag = dg ? uint32_t(atoi(dg + 1)) : 0u;
    if (!tile_form(A.tile_kib, A.tile_threads, A.tile_diag)) return bad();
  }
  const AblateState product;
  A.active = A.gather_threads || A.gather_grid || A.group || A.pieces || A.stream_lb ||
             A.small_piece || !A.gather_staged || A.value_sweep != product.value_sweep ||
             A.tile_kib != product.tile_kib || !A.tile_xcd ||
             A.tile_threads != product.tile_threads || A.tile_diag;
  return ctx;
}

// okv_close's hook (the arms' buffers release themselves with the context).
void ablate_close(okv_ctx* ctx) {
  AblateState& A = ctx->ab;
  if (A.stream2) {
    (void)hipStreamSynchronize(A.stream2);
    (void)hipStreamDestroy(A.stream2);
  }
  for (hipEvent_t& ev : A.ev_piece)
    if (ev) (void)hipEventDestroy(ev);
}

// Diagnostic (tile-pass phase probe, OKV_TILE=...d3 / d7): copy the probe buffer to host.
extern "C" int okv_debug_probe(okv_ctx* ctx, void* host, size_t bytes) {
  if (!ctx || !ctx->ab.d_vsrc.data()) return OKV_E_ARG;
  OKV_HIP(hipMemcpy(host, ctx->ab.d_vsrc.data(), std::min(bytes, ctx->ab.d_vsrc.bytes()),
                    hipMemcpyDeviceToHost));
  return OKV_OK;
}

// The value sweep's launch: OKV_VALUE_SWEEP = form, tiles per workgroup, loads
// (1|2|4 unaligned; 5|6|7 aligned with lane shuffles).
void launch_value_sweep(okv_ctx* ctx, uint32_t form, uint64_t tiles, const SweepParams& S) {
  static const struct {
    uint32_t form, per;
    void (*kernel)(SweepParams);
  } kForms[] = {{1, 1, okv_value_sweep_kernel<1>},       {2, 2, okv_value_sweep_kernel<2>},
                {4, 4, okv_value_sweep_kernel<4>},       {5, 4, okv_value_sweep_kernel<4, true>},
                {6, 2, okv_value_sweep_kernel<2, true>}, {7, 3, okv_value_sweep_kernel<3, true>}};
  for (const auto& f : kForms)
    if (f.form == form)
      hipLaunchKernelGGL(f.kernel, dim3(uint32_t((tiles + f.per - 1) / f.per)), dim3(256), 0,
                         ctx->stream, S);
}

// decode_device's hook: the decode of a context on which some knob selects an
// arm (AblateState::active), from prepare's Work on: the product dispatcher's
// steps with the arm's kernels in place of the route's.  Large blocks: block /
// tile (whole or in two pieces) / sweep / staged gather; small ones: fused /
// stream / group / small pieces / the gather kernels.
int ablate_decode(okv_ctx* ctx, const Work& w, uint32_t nblk, int comp, okv_decode_out* o,
                  uint32_t flags) {
  AblateState& A = ctx->ab;
  const bool index_only = flags & OKV_F_INDEX_ONLY;
  const uint32_t gt = A.gather_threads ? A.gather_threads : gather_threads(w, nblk);
  const bool fused = ctx->fused && nblk && nblk <= ctx->fused_max && gt == 64;
  // stream: measured 9.2 vs 1.38 ms per CM segment of 386 K blocks (every
  // block's look-back walks back to an inclusive frontier that lags by the
  // blocks in flight)
  const bool stream = A.stream_lb && ctx->fused && nblk > ctx->fused_max && gt == 64;
  const bool large = nblk && !fused && !stream && gt == 256;
  // group: CM decode stage 5.9-6.8 vs 4.1 ms for passes 1-3 (DESIGN.md 17.4)
  const bool group = A.group && nblk && !fused && !stream && !large && !index_only;
  // block: OKV_VALUE_SWEEP=9, 10 (512 threads), 11 (diagnostic: the prefix
  // from okv_count_kernel instead of the look-back)
  const bool block = large && A.value_sweep >= 9 && !index_only && !w.pre;
  const bool block_diag = block && A.value_sweep == 11;
  const bool tile = large && !block && A.value_sweep >= 8;
  const bool sweep = large && !tile && !block && A.value_sweep && !index_only &&
                     A.gather_staged && o->row_cap < (uint64_t(1) << 32);
  const TileGeo geo = tile ? tile_geo(ctx, w, nblk, index_only, uint64_t(A.tile_kib) << 10)
                           : TileGeo{1, ~0ull};
  ctx->span_hint = SpanHint{};
  int rc;
  uint16_t* rt_kl = nullptr;
  if ((rc = ensure_blocks(ctx, nblk))) return rc;
  if ((tile || sweep) && (rc = ensure_hdr(ctx, nblk, &rt_kl))) return rc;
  CopyParams P = copy_params(ctx, w, nblk, index_only, rt_kl, geo.span_cap, *o);
  const uint32_t b0 = tile && A.pieces ? piece_split(nblk) : 0u;
  // small blocks in pieces of ~small_piece bytes (OKV_SMALL_PIECE_MB): count
  // then gather per piece, the gather reading what the count just read
  uint32_t spn = 0;
  if (!fused && !stream && !large && !group && nblk && A.small_piece &&
      w.seg_bytes > A.small_piece)
    spn = std::max<uint32_t>(kTile, uint32_t(uint64_t(nblk) * A.small_piece / w.seg_bytes) &
                                        ~uint32_t(kTile - 1));
  if (spn >= nblk) spn = 0;
  // passes 1-2, unless the arm's kernel does them itself
  bool early_big = false;  // (see decode_device)
  if (fused || stream || group || spn || (block && !block_diag)) {
    if (group) {
      rc = ensure_group(ctx, (nblk + kGroup - 1) / kGroup);
    } else if (spn) {  // the counts run piece by piece with the gathers below
      rc = reserve(ctx, A.d_ptot, 2);
    } else {
      rc = ensure_fused(ctx, nblk);
    }
    if (rc) return rc;
    prof_mark(ctx, 2);
    prof_mark(ctx, 3);
  } else if (b0) {
    if ((rc = launch_plan_pieces(ctx, w, nblk, b0, o->row_start, rt_kl, geo.span_cap))) return rc;
  } else {
    if ((rc = launch_plan(ctx, w, nblk, o->row_start, true, rt_kl, geo.span_cap))) return rc;
    early_big = nblk != 0;
    if (!early_big) prof_mark(ctx, 3);
  }
  uint64_t sw_tiles = 0;
  if (sweep) {
    sw_tiles = (o->val_cap + kSwTile - 1) / kSwTile;
    const uint64_t rows = std::max<uint64_t>(o->row_cap, 1);
    if ((rc = reserve(ctx, A.d_vsrc, rows * 24 + 256)) ||
        (rc = reserve(ctx, A.d_vtile, sw_tiles + 4)))
      return rc;
    // [row] u64 sources, then [row] 16-byte boundary chunks
    P.vsrc = reinterpret_cast<uint64_t*>(A.d_vsrc.data());
    P.bchunk = reinterpret_cast<uint4*>(A.d_vsrc.data() + ((rows * 8 + 255) & ~255ull));
    P.vtile = A.d_vtile.data();
  }
  const uint32_t gather = tile    ? OKV_PATH_TILE
                          : sweep ? OKV_PATH_SWEEP | OKV_PATH_STAGED
                          : gt == 256 && A.gather_staged && !index_only ? OKV_PATH_STAGED
                          : gt == 64 && A.gather_staged                 ? OKV_PATH_SMALL
                                                                        : OKV_PATH_GATHER;
  ctx->last_path = path_bits(w, comp, index_only,
                             !nblk    ? 0u
                             : fused  ? OKV_PATH_FUSED
                             : stream ? OKV_PATH_STREAM
                                      : OKV_PATH_BIG | (group ? OKV_PATH_GROUP : gather));
  if (early_big) {
    launch_big(ctx, P);
    OKV_HIP(hipGetLastError());
    prof_mark(ctx, 3);
  }
  if ((rc = chain_wait(ctx))) return rc;
  if (!nblk) return finish_decode(ctx, o, flags);
  // pass 3
  const dim3 g(A.gather_grid ? std::min<uint32_t>(nblk, A.gather_grid) : nblk);
  if (block_diag) {
    hipLaunchKernelGGL((okv_block_kernel<1024, false>), dim3(nblk), dim3(1024), 0, ctx->stream, P,
                       FusedParams{});
  } else if (fused || stream || block) {
    const FusedParams F = fused_params(ctx, w);
    if (block && A.value_sweep == 10)
      hipLaunchKernelGGL(okv_block_kernel<512>, dim3(nblk), dim3(512), 0, ctx->stream, P, F);
    else if (block)
      hipLaunchKernelGGL(okv_block_kernel<1024>, dim3(nblk), dim3(1024), 0, ctx->stream, P, F);
    else if (stream)
      hipLaunchKernelGGL(okv_decode_stream_kernel, dim3(nblk), dim3(64), 0, ctx->stream, P, F);
    else
      hipLaunchKernelGGL(okv_decode_fused_kernel, dim3(nblk), dim3(64), 0, ctx->stream, P, F);
    const hipError_t le = hipGetLastError();
    // (nothing ran: the counters keep their value, so f_base must too)
    if (le != hipSuccess) return set_err(ctx, OKV_E_HIP, "okv_decode_fused_kernel launch", le);
    // the stream / block arms advance both counters by nblk once the grid
    // completes; the fused kernel uses none
    if (stream || block) ctx->f_base += nblk;
    if (!block) ctx->big_slot ^= 1u;  // the kernel zeroed the other slot (see big_counter)
  } else if (group) {
    A.g_epoch = (A.g_epoch + 1) & 0x3fffffffu;
    if (!A.g_epoch) A.g_epoch = 1;  // (a zero tag would match the zeroed flags)
    const GroupParams G{w.pre,           ctx->d_cnt.data(), ctx->d_lp.data(),
                        ctx->d_tile_pre.data(), A.g_flag.data(), A.g_agg.data(),
                        A.g_incl.data(), A.g_epoch,         ctx->d_tot.data(),
                        big_counter(ctx, 1)};
    hipLaunchKernelGGL(okv_group_kernel, dim3((nblk + kGroup - 1) / kGroup), dim3(kThreads), 0,
                       ctx->stream, P, G);
    OKV_HIP(hipGetLastError());
    ctx->big_slot ^= 1u;  // the kernel zeroed the other slot (see big_counter)
  } else if (tile) {
    if ((A.tile_diag >= 3 && A.tile_diag <= 5) || A.tile_diag == 7) {
      // phase probe: 8 timestamps per 256th workgroup
      const size_t n = (size_t(nblk) * geo.tpb / 256 + 1) * 64;
      if ((rc = reserve(ctx, A.d_vsrc, n))) return rc;
      P.vsrc = reinterpret_cast<uint64_t*>(A.d_vsrc.data());
    }
    if (b0) {  // the first piece's tile pass, then the second's after its walk
      launch_tile(ctx, piece_params(P, 0, b0), geo);
      OKV_HIP(hipStreamWaitEvent(ctx->stream, A.ev_piece[1], 0));
      launch_tile(ctx, piece_params(P, b0, nblk - b0), geo);
    } else {
      launch_tile(ctx, P, geo);
    }
  } else if (sweep) {
    // per-block rows + keys (one wave per block), then the value sweep
    hipLaunchKernelGGL(okv_rows_kernel, g, dim3(64), 0, ctx->stream, P);
    if (sw_tiles)
      launch_value_sweep(ctx, A.value_sweep, sw_tiles,
                         SweepParams{w.seg, w.seg_bytes, o->val_off, o->val_len, P.vsrc, P.vtile,
                                     P.bchunk, o->val_arena, ctx->d_tot.data(), P.big_count,
                                     o->row_cap, o->key_cap, o->val_cap});
    // the whole pass when the sweep is unsafe on device (big blocks,
    // capacity); otherwise every workgroup returns at once (small grid)
    hipLaunchKernelGGL((okv_gather_staged_kernel<kThreads>), dim3(std::min<uint32_t>(nblk, 2048)),
                       dim3(kThreads), 0, ctx->stream, P);
  } else if (gt == 256 && A.gather_staged && !index_only) {
    hipLaunchKernelGGL((okv_gather_staged_kernel<kThreads>), g, dim3(kThreads), 0, ctx->stream, P);
  } else if (spn && A.gather_staged) {
    Totals* pt = A.d_ptot.data();
    const Totals* base = nullptr;
    for (uint32_t p0 = 0, k = 0; p0 < nblk; p0 += spn, ++k) {
      const uint32_t n = std::min(spn, nblk - p0);
      Totals* tot = p0 + n == nblk ? ctx->d_tot.data() : pt + (k & 1);
      launch_count_piece(ctx, ctx->stream, w, p0, n, o->row_start, base, tot, k == 0);
      hipLaunchKernelGGL(okv_gather_small_kernel, dim3(n), dim3(64), 0, ctx->stream,
                         piece_params(P, p0, n));
      base = tot;
    }
    ctx->big_slot ^= 1u;  // the first count launch zeroed the other slot
  } else if (gt == 64 && A.gather_staged) {
    hipLaunchKernelGGL(okv_gather_small_kernel, g, dim3(64), 0, ctx->stream, P);
  } else if (gt == 64) {
    hipLaunchKernelGGL(okv_gather_kernel<64>, g, dim3(64), 0, ctx->stream, P);
  } else {
    hipLaunchKernelGGL(okv_gather_kernel<kThreads>, g, dim3(kThreads), 0, ctx->stream, P);
  }
  if (!block && !early_big) launch_big(ctx, P);  // (the block kernel decodes every block itself)
  OKV_HIP(hipGetLastError());
  return finish_decode(ctx, o, flags);
}
