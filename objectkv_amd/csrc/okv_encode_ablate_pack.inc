// Ablation build only (#included by okv_encode.hip under -DOKV_ABLATE): the
// pack launch's measured variants, chosen by environment knobs
// (tools/ablate_enc.py, tools/c4_arms.sh):
//   OKV_ENC_VARIANT  arms of the record-major LDS kernel (okv_enc_pack_lds_arm_kernel<.., V>),
//                    for records of <= 512 bytes on average:
//                      0   row positions from the row prefix, not the workgroup scan
//                      4   7 without the block hashes (no FirstKey copies either)
//                      5   headers only: no key or value bytes are read
//                      6   keys and values loaded but not written to LDS
//                      7   the product kernel itself (okv_enc_pack_lds_kernel)
//                      8   7 with registers capped at 64 for 8 waves per SIMD (it spills)
//                      9   7 with wave 0 hashing the raw image while waves 1-3 store
//                          it: no pre-multiplied round inputs, no second barrier
//                      10  only with OKV_ENC_IMAGE=32768 (below); alone it is 0
//                    and of the chunk-major region kernel (okv_enc_pack_region_arm_kernel<V>),
//                    for larger records:
//                      1   the LDS tables only, nothing stored
//                      2   the tables, then each chunk's record index stored, not its bytes
//                      3   the product's large-record launch (pack_large) for every
//                          record size
//   OKV_ENC_IMAGE    the record-major kernel's LDS image size:
//                      8192 / 12288 / 32768   with V = 0 and 256 threads
//                      65536                  with V = 7 and 1 024 threads: one wave
//                                             hashes 16 blocks with all 64 lanes
//                      32768 with OKV_ENC_VARIANT=10   with V = 7 and 512 threads:
//                                             one wave hashes 8 blocks
//   OKV_ENC_META_FUSED=1  with OKV_ENC_VARIANT=7 or unset: the meta index entries
//                    written by the pack kernel (kMeta), not by the meta kernel;
//   OKV_ENC_NO_FK=1  the product launch without the FirstKey copies (the meta
//                    kernel then reads each block's first line from the segment).
// With none of them set, *handled stays false and enc_write runs the product
// launch (enc_pack).
//
// The arm kernels are the parameterised bodies the product kernels were cut
// from: a frozen record of the experiments, which need not track the product.

template <int V>  // 1 tables only, 2 tables + each chunk's record index stored
__global__ __launch_bounds__(kThreads) void okv_enc_pack_region_arm_kernel(PackParams P,
                                                                           uint64_t nb,
                                                                           uint32_t G) {
  __shared__ RegionSmem sm;
  const uint64_t k0 = uint64_t(blockIdx.x) * G;
  const uint32_t g = uint32_t(std::min<uint64_t>(G, nb - k0));
  const uint64_t O0 = P.desc[k0].offset;
  const Desc dl = P.desc[k0 + g - 1];
  const uint64_t nq = (dl.offset + dl.block_size - O0) >> 4;
  if (threadIdx.x <= g) {
    const uint32_t t = threadIdx.x;
    const uint64_t f = P.first[k0 + t];
    sm.bfirst[t] = f;
    if (t < g) {
      sm.brel[t] = P.desc[k0 + t].offset - O0;
      sm.bbase[t] = Pg(P.pl, P.tp, int64_t(f) - 1);
    }
  }
  __syncthreads();
  const uint64_t R0 = sm.bfirst[0];
  const uint32_t nrow = uint32_t(sm.bfirst[g] - R0);
  for (uint32_t i = threadIdx.x; i < nrow; i += kThreads) {
    const uint64_t r = R0 + i;
    const uint32_t lo = region_block(sm.bfirst, g, r);
    sm.out[i] = sm.brel[lo] + Pg(P.pl, P.tp, int64_t(r) - 1) - sm.bbase[lo];
    sm.ko[i] = P.key_off[r];
    sm.kl[i] = P.key_len[r];
    sm.vo[i] = P.val_off[r];
    sm.vl[i] = P.val_len[r];
  }
  if (threadIdx.x == 0) sm.out[nrow] = nq << 4;
  __syncthreads();
  // chunk q belongs to the record whose span [out[i], out[i+1]) holds byte 16q
  for (uint32_t i = threadIdx.x; i < nrow; i += kThreads) {
    const uint32_t qa = uint32_t((sm.out[i] + 15) >> 4), qb = uint32_t((sm.out[i + 1] + 15) >> 4);
    for (uint32_t q = qa; q < qb; ++q) sm.qrow[q] = uint16_t(i);
  }
  __syncthreads();
  auto rec = [&](uint64_t i) {
    RecInfo r;
    r.rs = sm.out[i];
    r.ko = sm.ko[i];
    r.vo = sm.vo[i];
    r.kl = sm.kl[i];
    r.vl = sm.vl[i];
    return r;
  };
  uint8_t* dst = P.seg + O0;
  if (V == 1) return;
  for (uint32_t q = threadIdx.x; q < nq; q += kThreads) {
    const uint64_t pos = uint64_t(q) << 4;
    if (V == 2)
      *reinterpret_cast<uint4*>(dst + pos) = make_uint4(sm.qrow[q], 0, 0, 0);
    else
      *reinterpret_cast<uint4*>(dst + pos) = assemble_chunk(P, pos, sm.qrow[q], nrow, rec);
  }
}

// V (OKV_ENC_VARIANT): 0 row positions from the row prefix; 4 no hash; 5 headers
// only; 6 loads without LDS writes; 7 row positions by a workgroup scan, no pl
// reads (what the product kernel does); 8 and 9 below.
// kMeta (OKV_ENC_META_FUSED=1): the meta index entries written here too
// (measured slower: 5.16-5.30 vs 4.31-4.39 ms pack, + 0.23 ms meta kernel saved).
template <uint32_t IMG, int V = 0, bool kMeta = false, uint32_t NT = kThreads>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(V == 8 ? 8 : 1)))
void okv_enc_pack_lds_arm_kernel(PackParams P, uint64_t nb, uint32_t G) {
  // V == 7 takes 70 registers, 7 waves per SIMD; V == 8 is the same code
  // capped at 64 registers for 8 waves: it spills (9 registers) and measured
  // 4.88 vs 3.85 ms (profiles/r3/r3g/ablate_enc.log)
  // V == 9: 7 with the block hashes computed by wave 0 from the raw image
  // while waves 1-3 store it (no second barrier, no precompute)
  constexpr bool kOverlap = V == 9;
  constexpr int VL = (V == 8 || V == 9) ? 7 : V;
  __shared__ uint4 img4[IMG / 16];
  __shared__ uint64_t bfirst[kMaxRegion + 1], brel[kMaxRegion], bbase[kMaxRegion];
  __shared__ uint32_t slim[kMaxRegion], blen[kMaxRegion];  // end of whole stripes, BlockSize
  __shared__ uint64_t borig[kMaxRegion], bcsz[kMaxRegion], bmoff[kMaxRegion];
  __shared__ uint32_t bfkl[kMaxRegion];  // key length of each block's first row (its FirstKey)
  uint32_t* img = reinterpret_cast<uint32_t*>(img4);
  const uint64_t k0 = uint64_t(blockIdx.x) * G;
  const uint32_t g = uint32_t(std::min<uint64_t>(G, nb - k0));
  // one HBM trip for everything that needs only the region's index: its
  // blocks' first rows and descriptors (clamped addresses, issued together;
  // round 4 waited for the region's extent before loading first[])
  const uint64_t frow = P.first[k0 + std::min<uint32_t>(threadIdx.x, g)];
  Desc dt{};
  if (threadIdx.x < 64) dt = P.desc[k0 + std::min<uint32_t>(threadIdx.x, g - 1)];
  const uint64_t O0 = P.desc[k0].offset;
  const Desc dl = P.desc[k0 + g - 1];
  const uint32_t nq = uint32_t((dl.offset + dl.block_size - O0) >> 4);
  if (threadIdx.x <= g) bfirst[threadIdx.x] = frow;
  for (uint32_t q = threadIdx.x; q < nq; q += NT) img4[q] = make_uint4(0, 0, 0, 0);
  if (threadIdx.x < 64) {  // g <= kMaxRegion = 64: wave 0
    const uint32_t t = threadIdx.x;
    uint64_t orig = 0;
    if (t < g) {  // (with first[], and the meta entry offset)
      brel[t] = dt.offset - O0;
      blen[t] = uint32_t(dt.block_size);
      slim[t] = uint32_t(dt.offset - O0 + (dt.block_size & ~uint64_t(31)));
      orig = dt.original_size;
      if constexpr (kMeta) {
        borig[t] = orig;
        bcsz[t] = dt.compressed_size;
        bmoff[t] = P.moff[k0 + t];
      }
    }
    // each block's start in the region's row stream: the OriginalSizes before it
    const uint64_t incl = wave_incl_scan(orig, int(t));
    if (t < g) bbase[t] = incl - orig;
  }
  __shared__ uint32_t s_wt[2][NT / 64];  // VL == 7: per-wave record-size totals
  __syncthreads();
  const uint64_t R0 = bfirst[0], R1 = bfirst[g];
  const uint64_t abs0 = VL == 7 ? 0 : Pg(P.pl, P.tp, int64_t(R0) - 1);
  uint32_t carry = 0;  // VL == 7: image bytes of the rows before this pass
  for (uint64_t base = R0; base < R1; base += NT) {  // uniform trip count (VL == 7 barriers)
    const uint64_t r = base + threadIdx.x;
    const bool live = r < R1;
    uint32_t kl = 0, vl = 0;
    uint64_t ko = 0, vo = 0;
    if (live) {
      kl = P.key_len[r];
      vl = P.val_len[r];
      ko = P.key_off[r];
      vo = P.val_off[r];
    }
    uint32_t srel = 0;  // VL == 7: region-relative start of record r's row stream
    if constexpr (VL == 7) {
      // exclusive scan of the record sizes in row order (< IMG bytes: u32)
      const uint32_t sz = live ? 6 + kl + vl : 0u;
      const uint32_t inc = wave_scan_dpp(sz);
      const uint32_t wave = threadIdx.x >> 6, par = uint32_t((base - R0) / NT) & 1;
      if ((threadIdx.x & 63) == 63) s_wt[par][wave] = inc;
      __syncthreads();
      uint32_t before = carry, tot = 0;
#pragma unroll
      for (uint32_t w = 0; w < NT / 64; ++w) {
        const uint32_t t = s_wt[par][w];
        before += w < wave ? t : 0u;
        tot += t;
      }
      srel = before + inc - sz;
      carry += tot;
    }
    if (!live) continue;
    const uint32_t lo = region_block(bfirst, g, r);
    if (kMeta && r == bfirst[lo]) bfkl[lo] = kl;
    // (the other arms: the row's absolute row-stream position from the row
    // prefix, less the block's -- the region's first row's absolute position
    // abs0 plus the block's region-relative base)
    const uint32_t d = VL == 7 ? uint32_t(brel[lo] + srel - (bbase[lo] - bbase[0]))
                              : uint32_t(brel[lo] + Pg(P.pl, P.tp, int64_t(r) - 1) -
                                         (abs0 + bbase[lo]));
    if (VL == 5) {
      lds_or16(img, d, make_uint4(kl | (vl << 16), vl >> 16, 0, 0));
    } else if (VL == 6 && kl <= 64 && vl <= 64) {
      const Lines5 K = load_lines5(P.key_arena + ko, kl);
      const Lines5 Vl = load_lines5(P.val_arena + vo, vl);
      uint32_t x = 0;
#pragma unroll
      for (int t = 0; t < 5; ++t) x ^= K.l[t].x ^ K.l[t].w ^ Vl.l[t].y ^ Vl.l[t].z;
      lds_or16(img, d, make_uint4(kl | (vl << 16), vl >> 16, x == 0x9e3779b9u ? 1u : 0u, 0));
    } else if (kl <= 64 && vl <= 64) {  // all source lines of the record in flight at once
      const Lines5 K = load_lines5(P.key_arena + ko, kl);
      const Lines5 Vl = load_lines5(P.val_arena + vo, vl);
      lds_or16(img, d, make_uint4(kl | (vl << 16), vl >> 16, 0, 0));
      lds_put5(img, d + 6, K, kl);
      if (vl) lds_put5(img, d + 6 + kl, Vl, vl);
    } else {
      lds_or16(img, d, make_uint4(kl | (vl << 16), vl >> 16, 0, 0));
      lds_copy_field(img, d + 6, P.key_arena + ko, kl);
      if (vl) lds_copy_field(img, d + 6 + kl, P.val_arena + vo, vl);
    }
  }
  __syncthreads();
  uint4* dst = reinterpret_cast<uint4*>(P.seg + O0);
  if constexpr (kOverlap) {
    if (threadIdx.x >= 64) {
      for (uint32_t q = threadIdx.x - 64; q < nq; q += NT - 64) dst[q] = img4[q];
      return;
    }
  } else {
  // the image stored and the XXH64 round inputs pre-multiplied in place, as
  // pack_store (okv_encode.hip) describes
  for (uint32_t q = threadIdx.x; q < nq; q += NT) {
    const uint4 v = img4[q];
    store_nt16(&dst[q], v);
    if (VL == 4) continue;
    const uint32_t p = q << 4;
    const uint32_t lo = region_block(brel, g, p);
    if (P.fk && p < uint32_t(brel[lo]) + kFkStride && p + 16 <= uint32_t(brel[lo]) + blen[lo])
      *reinterpret_cast<uint4*>(P.fk + (k0 + lo) * kFkStride + (p - uint32_t(brel[lo]))) = v;
    if constexpr (kMeta) {  // FirstKey bytes of the block's meta entry (block_stat.go:31-33)
      const uint32_t ks = uint32_t(brel[lo]) + 6, ke = ks + bfkl[lo];
      const uint32_t a0 = max(p, ks), a1 = min(p + 16, ke);
      uint8_t* m = P.meta + bmoff[lo] + 2 - ks;
      for (uint32_t x = a0; x < a1; ++x) m[x] = uint8_t(dword_at(v, x - p));
    }
    if (p + 16 <= slim[lo]) {
      const uint64_t a = ((uint64_t(v.y) << 32) | v.x) * XP2;
      const uint64_t c = ((uint64_t(v.w) << 32) | v.z) * XP2;
      img4[q] = make_uint4(uint32_t(a), uint32_t(a >> 32), uint32_t(c), uint32_t(c >> 32));
    }
  }
  if (VL == 4) return;
  // only LDS has to be ordered here (a __syncthreads would also wait for the
  // image's global stores)
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  // BlockStat.Hash = XXH64 of the padded block (segment_writer.go:185), from
  // the image: four lanes per block own XXH64's four accumulators.
  if (threadIdx.x < 4 * g) {
    const uint32_t b = threadIdx.x >> 2, q = threadIdx.x & 3;
    const uint32_t boff = uint32_t(brel[b]);
    const uint64_t len = blen[b];
    const uint64_t* w64 = reinterpret_cast<const uint64_t*>(img4) + (boff >> 3);
    uint64_t acc = (q == 0) ? XP1 + XP2 : (q == 1) ? XP2 : (q == 2) ? 0 : 0 - XP1;
    const uint32_t nstripe = uint32_t(len / 32);
    uint32_t st = 0;
    for (; st + 8 <= nstripe; st += 8) {  // 8 LDS reads ahead of the round chain
      uint64_t x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = w64[4 * (st + u) + q];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = kOverlap ? xround(acc, x[u]) : xround_pre(acc, x[u]);
    }
    for (; st < nstripe; ++st)
      acc = kOverlap ? xround(acc, w64[4 * st + q]) : xround_pre(acc, w64[4 * st + q]);
    const int lane = threadIdx.x & 63;
    const uint64_t a1 = __shfl(acc, (lane & ~3) + 1, 64);
    const uint64_t a2 = __shfl(acc, (lane & ~3) + 2, 64);
    const uint64_t a3 = __shfl(acc, (lane & ~3) + 3, 64);
    if (q == 0) {
      uint64_t h;
      if (len >= 32) {
        h = rotl64(acc, 1) + rotl64(a1, 7) + rotl64(a2, 12) + rotl64(a3, 18);
        h = (h ^ xround(0, acc)) * XP1 + XP4;
        h = (h ^ xround(0, a1)) * XP1 + XP4;
        h = (h ^ xround(0, a2)) * XP1 + XP4;
        h = (h ^ xround(0, a3)) * XP1 + XP4;
      } else {
        h = XP5;
      }
      h += len;
      const uint8_t* bytes = reinterpret_cast<const uint8_t*>(img4) + boff;
      uint32_t t = nstripe * 32;
      for (; t + 8 <= len; t += 8) {
        h ^= xround(0, w64[t / 8]);
        h = rotl64(h, 27) * XP1 + XP4;
      }
      if (t + 4 <= len) {
        const uint32_t v = uint32_t(bytes[t]) | (uint32_t(bytes[t + 1]) << 8) |
                           (uint32_t(bytes[t + 2]) << 16) | (uint32_t(bytes[t + 3]) << 24);
        h ^= uint64_t(v) * XP1;
        h = rotl64(h, 23) * XP2 + XP3;
        t += 4;
      }
      for (; t < len; ++t) {
        h ^= uint64_t(bytes[t]) * XP5;
        h = rotl64(h, 11) * XP1;
      }
      h ^= h >> 33;
      h *= XP2;
      h ^= h >> 29;
      h *= XP3;
      h ^= h >> 32;
      P.hash[k0 + b] = h;
      if constexpr (kMeta) {  // the rest of the entry: u16 len(FirstKey), then 5 x u64 (:27-42)
        uint8_t* m = P.meta + bmoff[b];
        const uint32_t kl = bfkl[b];
        put_le(m, kl, 2);
        m += 2 + kl;
        put_le(m, O0 + boff, 8);
        put_le(m + 8, len, 8);
        put_le(m + 16, borig[b], 8);
        put_le(m + 24, bcsz[b], 8);
        put_le(m + 32, h, 8);
      }
    }
  }
}

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
  const bool aligned = pack_aligned(o, seg);
  const int EV = evar ? atoi(evar) : 7;
  const int eimg_v = eimg ? atoi(eimg) : 0;
  const uint32_t img = (eimg_v == 32768 || eimg_v == 8192 || eimg_v == 12288 || eimg_v == 65536)
                            ? uint32_t(eimg_v)
                            : kImage;
  const uint64_t GLa = std::min<uint64_t>(kMaxRegion, img / std::max<uint64_t>(pl.bmax, 1));
  int rc;
  if (aligned && GLa >= 1 && pl.avg_rec <= 512 && EV != 3) {
    // the record-major kernel's arm, its workgroup size, and whether it reads
    // the row prefix (every V but 7, 8 and 9)
    void (*kern)(PackParams, uint64_t, uint32_t) = okv_enc_pack_lds_arm_kernel<kImage>;
    uint32_t nt = kThreads;
    bool prefix = true;
    if (img == 65536) {
      kern = okv_enc_pack_lds_arm_kernel<65536, 7, false, 1024>;
      nt = 1024;
      prefix = false;
    } else if (img == 32768 && EV == 10) {
      kern = okv_enc_pack_lds_arm_kernel<32768, 7, false, 512>;
      nt = 512;
      prefix = false;
    } else if (img == 32768) {
      kern = okv_enc_pack_lds_arm_kernel<32768>;
    } else if (img == 8192) {
      kern = okv_enc_pack_lds_arm_kernel<8192>;
    } else if (img == 12288) {
      kern = okv_enc_pack_lds_arm_kernel<12288>;
    } else if (EV == 7 && meta_fused) {
      kern = okv_enc_pack_lds_arm_kernel<kImage, 7, true>;
      prefix = false;
      pp.meta = seg + pl.data_bytes;
      *meta_done = true;
    } else if (EV == 7) {
      kern = okv_enc_pack_lds_kernel;  // the product kernel
      prefix = false;
    } else if (EV == 4) {
      kern = okv_enc_pack_lds_arm_kernel<kImage, 4>;
    } else if (EV == 5) {
      kern = okv_enc_pack_lds_arm_kernel<kImage, 5>;
    } else if (EV == 6) {
      kern = okv_enc_pack_lds_arm_kernel<kImage, 6>;
    } else if (EV == 8) {
      kern = okv_enc_pack_lds_arm_kernel<kImage, 8>;
      prefix = false;
    } else if (EV == 9) {
      kern = okv_enc_pack_lds_arm_kernel<kImage, 9>;
      prefix = false;
    }
    if (prefix) {
      if ((rc = enc_row_prefix(ctx, e, R, o.threshold_bytes))) return rc;
      pp.pl = e->pl.data();  // (allocated by the call above)
      pp.tp = e->tile_pre.data();
    }
    hipLaunchKernelGGL(kern, dim3(ceil_div(pl.nb, GLa)), dim3(nt), 0, ctx->stream, pp, pl.nb,
                       uint32_t(GLa));
    *hashed = true;
    return OKV_OK;
  }
  const uint64_t G = pack_region_blocks(pl);
  if (aligned && G >= 1 && (EV == 1 || EV == 2)) {  // the region kernel's diagnostic arms
    if ((rc = enc_row_prefix(ctx, e, R, o.threshold_bytes))) return rc;
    pp.pl = e->pl.data();
    pp.tp = e->tile_pre.data();
    hipLaunchKernelGGL(
        EV == 1 ? okv_enc_pack_region_arm_kernel<1> : okv_enc_pack_region_arm_kernel<2>,
        dim3(ceil_div(pl.nb, G)), dim3(kThreads), 0, ctx->stream, pp, pl.nb, uint32_t(G));
    return OKV_OK;
  }
  return pack_large(ctx, e, R, o, pl, seg, pp);  // (3, and every large-record launch)
}
