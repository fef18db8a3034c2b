// Ablation build only (#included by okv_encode.hip under -DOKV_ABLATE): the
// host side of the single-pass plan arm (OKV_ENC_ONEPASS=1).
// E1-E9 in one launch (okv_enc_plan_kernel).  *general = true when the shape
// needs the general kernels (a block longer than kFuseLook rows): the caller
// then runs enc_plan.
int enc_plan_fast(okv_ctx* ctx, EncScratch* e, const DevRows& R, const okv_encode_opts& o,
                  Plan* pl, uint64_t* bad_row, bool* general) {
  const uint64_t n = R.n;
  const uint64_t nch = (n + kETile - 1) / kETile;
  int rc;
  *general = false;
  e->have_pl = false;
  bool fresh = false;
  if ((rc = reserve(ctx, e->p_flag, nch, &fresh))) return rc;
  if (fresh) OKV_HIP(hipMemsetAsync(e->p_flag.data(), 0, e->p_flag.bytes(), ctx->stream));
  if ((rc = reserve(ctx, e->p_inc, nch * sizeof(PlanChunk))) ||
      (rc = reserve(ctx, e->p_tab, nch * kFuseLook)) || (rc = reserve(ctx, e->p_jlim, nch)))
    return rc;
  fresh = false;
  if ((rc = reserve(ctx, e->p_ctr, 1, &fresh))) return rc;
  if (fresh) {
    OKV_HIP(hipMemsetAsync(e->p_ctr.data(), 0, e->p_ctr.bytes(), ctx->stream));
    e->p_base = 0;
  }
  // per-block outputs: the last capacity, or a guess (a block of 4 KiB holds
  // tens of small rows); a launch that finds more blocks is rerun once
  uint64_t cap = std::max<uint64_t>(e->first.capacity() ? e->first.capacity() - 1 : 0,
                                    n / 32 + 1024);
  cap = std::min<uint64_t>(cap, n);
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = ensure_blocks_enc(ctx, e, cap))) return rc;
    enc_mark(ctx, e, 0);
    hipLaunchKernelGGL(okv_enc_init_kernel, dim3(1), dim3(1), 0, ctx->stream, e->d_tot.data());
    PlanParams P;
    P.key_len = R.kl;
    P.val_len = R.vl;
    P.n = n;
    P.T = o.threshold_bytes;
    P.D = o.block_size;
    P.lz4 = o.compression == OKV_COMP_LZ4;
    P.bloom_extra = o.bloom ? 8 + o.bloom_len : 0;
    P.nch = nch;
    P.flag = e->p_flag.data();
    P.inc = reinterpret_cast<PlanChunk*>(e->p_inc.data());
    P.tab = e->p_tab.data();
    P.jlim = e->p_jlim.data();
    P.ctr = e->p_ctr.data();
    P.base = e->p_base;
    e->p_epoch = (e->p_epoch % 0x3fffffffu) + 1;  // never 0 (the zeroed flags)
    P.epoch = e->p_epoch;
    P.cap = cap;
    P.first = e->first.data();
    P.desc = e->desc.data();
    P.moff = e->moff.data();
    P.tot = e->d_tot.data();
    hipLaunchKernelGGL(okv_enc_plan_kernel, dim3(uint32_t(nch)), dim3(kThreads), 0, ctx->stream,
                       P);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return set_err(ctx, OKV_E_HIP, "okv_enc_plan_kernel launch", le);
    e->p_base += nch;  // every workgroup claims one chunk
    if ((rc = read_enc_totals(ctx, e))) return rc;
    const EncTotals& t = *e->h_tot;
    if (t.far) {
      *general = true;
      return OKV_OK;
    }
    if (t.bad_row != kNone) {
      *bad_row = t.bad_row;
      return set_err(ctx, OKV_W_INVALID_KEY, "key cannot be empty (ErrInvalidKey)");
    }
    if (t.fault || t.nb == 0 || t.nb > n) return set_err(ctx, OKV_E_HIP, "encode: inconsistent plan");
    if (t.pad[0]) {  // more blocks than the guess: grow and rerun
      cap = t.nb;
      continue;
    }
    pl->nb = t.nb;
    pl->data_bytes = t.data_bytes;
    pl->head = t.head;
    pl->meta_bytes = t.head + t.meta_ent;
    pl->file_bytes = pl->data_bytes + pl->meta_bytes + 25;
    pl->last_raw = t.last_raw;
    pl->w = std::max<uint64_t>(1, t.wmax);
    pl->bmax = t.bmax;
    pl->avg_rec = t.total_raw / n;
    return OKV_OK;
  }
  return set_err(ctx, OKV_E_HIP, "encode: plan capacity");
}
