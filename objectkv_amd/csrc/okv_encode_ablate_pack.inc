// Ablation build only (#included by okv_encode.hip under -DOKV_ABLATE): the
// pack launch's measured variants, chosen by environment knobs
// (tools/ablate_enc.py, tools/c4_arms.sh):
//   OKV_ENC_VARIANT  4..9: okv_enc_pack_lds_kernel diagnostic arms (4 no hash,
//                    5 headers only, 6 loads without LDS writes, 8 = 7 with the
//                    hashes from the raw image, 9 = hashes by wave 0 beside the
//                    stores); 1, 2: the chunk-major region kernel's arms; 3: the
//                    region kernel for every record size;
//   OKV_ENC_IMAGE    8192 / 12288 / 32768: the LDS image size of the record-major
//                    kernel (V = 0: record positions from the row prefix); 65536:
//                    the product form (V = 7) on a 64 KiB image with 1 024 threads,
//                    so one wave hashes 16 blocks with all 64 lanes (with
//                    OKV_ENC_VARIANT=10 and 32768: 512 threads, 8 blocks);
//   OKV_ENC_META_FUSED=1: the meta entries written by the pack kernel;
//   OKV_ENC_NO_FK=1: the product launch without the FirstKey copies (the meta
//                    kernel then reads each block's first line from the segment).
// With none of them set, *handled stays false and enc_write runs the product
// launch (enc_pack).
int enc_pack_ablate(okv_ctx* ctx, EncScratch* e, const DevRows& R, const okv_encode_opts& o,
                    const Plan& pl, uint8_t* seg, PackParams& pp, bool* hashed, bool* meta_done,
                    bool* handled) {
  const char* evar = okv::knob("OKV_ENC_VARIANT");
  const char* eimg = okv::knob("OKV_ENC_IMAGE");
  const char* emeta = okv::knob("OKV_ENC_META_FUSED");
  const bool meta_fused = emeta && atoi(emeta);
  const char* nofk = okv::knob("OKV_ENC_NO_FK");
  if (nofk && atoi(nofk) && !evar && !eimg && !meta_fused) {
    bool fk_done = false;
    PackParams q = pp;
    q.fk = nullptr;  // (a null one is skipped by the kernel)
    *handled = true;
    return enc_pack(ctx, e, R, o, pl, seg, q, hashed, &fk_done);
  }
  if (!evar && !eimg && !meta_fused) return OKV_OK;
  *handled = true;
  const bool aligned = o.block_size % 16 == 0 && (reinterpret_cast<uintptr_t>(seg) & 15) == 0;
  const int EV = evar ? atoi(evar) : 7;
  const int eimg_v = eimg ? atoi(eimg) : 0;
  const uint32_t img = (eimg_v == 32768 || eimg_v == 8192 || eimg_v == 12288 || eimg_v == 65536)
                            ? uint32_t(eimg_v)
                            : kImage;
  const uint64_t GLa = std::min<uint64_t>(kMaxRegion, img / std::max<uint64_t>(pl.bmax, 1));
  const bool lds = aligned && GLa >= 1 && pl.avg_rec <= 512 && EV != 3;
  int rc;
  // every arm but the product's record-major kernel reads the row prefix
  if (!(lds && (EV == 7 || EV == 10) && (img == kImage || img == 65536 || img == 32768)) &&
      (rc = enc_row_prefix(ctx, e, R, o.threshold_bytes)))
    return rc;
  pp.pl = e->pl.data();  // (allocated by the call above)
  pp.tp = e->tile_pre.data();
  const dim3 blk(kThreads);
  if (lds) {
    const dim3 grid(ceil_div(pl.nb, GLa));
    if (img == 65536) {
      pp.fk = e->fk.data();
      hipLaunchKernelGGL((okv_enc_pack_lds_kernel<65536, 7, false, 1024>), grid, dim3(1024), 0,
                         ctx->stream, pp, pl.nb, uint32_t(GLa));
      *hashed = true;
      return OKV_OK;
    }
    if (img == 32768 && EV == 10) {  // 32 KiB image, 512 threads: one wave hashes 8 blocks
      pp.fk = e->fk.data();
      hipLaunchKernelGGL((okv_enc_pack_lds_kernel<32768, 7, false, 512>), grid, dim3(512), 0,
                         ctx->stream, pp, pl.nb, uint32_t(GLa));
      *hashed = true;
      return OKV_OK;
    }
    if (img == 32768)
      hipLaunchKernelGGL(okv_enc_pack_lds_kernel<32768>, grid, blk, 0, ctx->stream, pp, pl.nb,
                         uint32_t(GLa));
    else if (img == 8192)
      hipLaunchKernelGGL(okv_enc_pack_lds_kernel<8192>, grid, blk, 0, ctx->stream, pp, pl.nb,
                         uint32_t(GLa));
    else if (img == 12288)
      hipLaunchKernelGGL(okv_enc_pack_lds_kernel<12288>, grid, blk, 0, ctx->stream, pp, pl.nb,
                         uint32_t(GLa));
    else if (EV >= 4 && EV <= 9) {
      void (*kern)(PackParams, uint64_t, uint32_t) = EV == 4   ? okv_enc_pack_lds_kernel<kImage, 4>
                                                     : EV == 5 ? okv_enc_pack_lds_kernel<kImage, 5>
                                                     : EV == 6 ? okv_enc_pack_lds_kernel<kImage, 6>
                                                     : EV == 8 ? okv_enc_pack_lds_kernel<kImage, 8>
                                                     : EV == 9 ? okv_enc_pack_lds_kernel<kImage, 9>
                                                               : okv_enc_pack_lds_kernel<kImage, 7>;
      if (EV == 7 && meta_fused) {
        pp.meta = seg + pl.data_bytes;
        *meta_done = true;
        kern = okv_enc_pack_lds_kernel<kImage, 7, true>;
      }
      hipLaunchKernelGGL(kern, grid, blk, 0, ctx->stream, pp, pl.nb, uint32_t(GLa));
    } else {
      hipLaunchKernelGGL(okv_enc_pack_lds_kernel<kImage>, grid, blk, 0, ctx->stream, pp, pl.nb,
                         uint32_t(GLa));
    }
    *hashed = true;
    return OKV_OK;
  }
  const uint64_t G = pack_region_blocks(pl);
  if (aligned && G >= 1) {
    const int V = EV == 7 ? 0 : EV;
    const dim3 grid(ceil_div(pl.nb, G));
    if (V == 1)
      hipLaunchKernelGGL(okv_enc_pack_region_kernel<1>, grid, blk, 0, ctx->stream, pp, pl.nb,
                         uint32_t(G));
    else if (V == 2)
      hipLaunchKernelGGL(okv_enc_pack_region_kernel<2>, grid, blk, 0, ctx->stream, pp, pl.nb,
                         uint32_t(G));
    else
      hipLaunchKernelGGL(okv_enc_pack_region_kernel<0>, grid, blk, 0, ctx->stream, pp, pl.nb,
                         uint32_t(G));
  } else if (aligned) {
    hipLaunchKernelGGL(okv_enc_pack_kernel, dim3(uint32_t(pl.nb)), blk, 0, ctx->stream, pp);
  } else {
    const uint32_t g = std::min<uint64_t>(65536, (pl.data_bytes + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(okv_enc_pack_bytes_kernel, dim3(std::max<uint32_t>(g, 1)), blk, 0,
                       ctx->stream, pp, pl.nb, pl.data_bytes);
  }
  return OKV_OK;
}
