// okv_zstd_ablate_host.inc -- the zstd stage's A/B knobs and diagnostics.
// Included by okv_zstd.hip inside namespace okv::zst, in the ablation build
// (-DOKV_ABLATE) only; the product build has empty hooks in its place.
//
// Knobs, read from the environment at every zstd decode:
//   OKV_ZSTD_GENERAL=1     every block through the general kernel (A/B of the
//                          staged decoder; as OKV_OPEN_ZSTD_ONE_PASS)
//   OKV_ZSTD_PRO_GRID=n    prologue workgroups (default: one per block)
//   OKV_ZSTD_EXEC_GRID=n   executor workgroups (default: one per block)
//   OKV_ZSTD_HUF_BLOCKS=n  blocks per wave of the Huffman stream stage: 2, 8
//                          or 16 (anything else: the build's kHufBlocks)
//   OKV_ZSTD_PROF=1        per-stage milliseconds and the prologue's and the
//                          executor's phase cycle counters, printed to stderr
//                          after the decode (tools/zstd_prof.py); the executor
//                          grid is capped at its kExecGridMax counter slots

// The executor's phase counters: 16 slots per workgroup (blocks are strided
// over the grid), sized for the largest profiled grid.
constexpr uint32_t kExecGridMax = 16384;

// A context's diagnostic state (zst::Scratch::diag).
struct Diag {
  bool prof = false;                    // this decode is profiled
  uint32_t nblk = 0;
  hipEvent_t ev[5] = {};                // start, then one per diag_mark
  DevBuf<unsigned long long> eprof;     // [kExecGridMax][16] executor phase cycles
  DevBuf<unsigned long long> pprof;     // [16] prologue phase cycles
  std::vector<unsigned long long> hs;   // eprof on the host
};

inline uint32_t knob_u32(const char* name, uint32_t dflt) {
  const char* v = okv::knob(name);
  return v ? uint32_t(atoi(v)) : dflt;
}

// The knobs into the plan; a profiled decode starts its clock and zeroes the
// phase counters.
inline int diag_begin(okv_ctx* ctx, Diag& d, uint32_t nblk, Plan* p) {
  hipStream_t s = ctx->stream;
  d.prof = okv::knob("OKV_ZSTD_PROF") != nullptr;
  d.nblk = nblk;
  p->general = p->general || okv::knob("OKV_ZSTD_GENERAL") != nullptr;
  p->pro_grid = std::max(1u, std::min(nblk, knob_u32("OKV_ZSTD_PRO_GRID", nblk)));
  uint32_t egrid = knob_u32("OKV_ZSTD_EXEC_GRID", nblk);
  if (d.prof) egrid = std::min(egrid, kExecGridMax);
  p->exec_grid = std::min(nblk, std::max(egrid, 1u));
  const uint32_t hb = knob_u32("OKV_ZSTD_HUF_BLOCKS", kHufBlocks);
  if (hb == 16) p->huf = launch_huf<16>;
  if (hb == 8) p->huf = launch_huf<8>;
  if (hb == 2) p->huf = launch_huf<2>;
  if (!d.prof) return OKV_OK;
  for (auto& e : d.ev) (void)hipEventCreate(&e);
  (void)hipEventRecord(d.ev[0], s);
  int rc;
  if ((rc = reserve(ctx, d.eprof, 16 * kExecGridMax)) || (rc = reserve(ctx, d.pprof, 16)))
    return rc;
  p->eprof = d.eprof.data();
  p->pprof = d.pprof.data();
  (void)hipMemsetAsync(p->eprof, 0, 16 * 8 * kExecGridMax, s);
  (void)hipMemsetAsync(p->pprof, 0, 16 * 8, s);
  return OKV_OK;
}

// The three reports of a profiled decode.
inline void diag_report(okv_ctx* ctx, Diag& d) {
  (void)hipStreamSynchronize(ctx->stream);
  float t[4] = {};
  for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&t[k], d.ev[k], d.ev[k + 1]);
  fprintf(stderr,
          "[zstd prof] %u blocks: prologue+seqoff %.3f ms, sequences %.3f ms, executor %.3f ms, "
          "general %.3f ms\n",
          d.nblk, t[0], t[1], t[2], t[3]);
  for (auto& e : d.ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  d.hs.resize(16 * kExecGridMax);
  (void)hipMemcpy(d.hs.data(), d.eprof.data(), d.hs.size() * 8, hipMemcpyDeviceToHost);
  unsigned long long h[16] = {};
  for (uint32_t w = 0; w < kExecGridMax; ++w)
    for (int k = 0; k < 16; ++k) h[k] += d.hs[w * 16 + k];
  const double c = h[9] ? double(h[9]) : 1.0;
  fprintf(stderr,
          "[zstd exec] chunks %llu, cycles/chunk: load+scan %.0f map %.0f sources %.0f jump %.0f "
          "(rounds %.2f) gather %.0f commit %.0f\n",
          h[9], h[0] / c, h[1] / c, h[2] / c, h[3] / c, h[8] / c, h[4] / c, h[5] / c);
  unsigned long long pp[16] = {};
  (void)hipMemcpy(pp, d.pprof.data(), sizeof(pp), hipMemcpyDeviceToHost);
  const double nb = pp[13] ? double(pp[13]) : 1.0;
  fprintf(stderr,
          "[zstd pro] blocks %llu, cycles/block: whole %.0f literals %.0f (huffman tree %.0f) "
          "sequence tables %.0f\n",
          pp[13], pp[11] / nb, pp[0] / nb, pp[12] / nb, pp[10] / nb);
}

// k = 1: prologue, sequence offsets and streams launched and the sequence count
// read; 2: sequences; 3: executor; 4: general kernel and regrow.
inline void diag_mark(okv_ctx* ctx, Diag& d, int k) {
  if (!d.prof) return;
  (void)hipEventRecord(d.ev[k], ctx->stream);
  if (k == 4) diag_report(ctx, d);
}
