// okv_ctx.hpp -- the per-GPU context shared by the decode (okv_decode.hip), encode
// (okv_encode.hip), zstd (okv_zstd.hip), merge (okv_merge.hip) and batched GetRow
// (okv_get.hip, okv_snap.hip) translation units, the zstd encoder (okv_zstd_enc.hip) and the
// range seek and gather (okv_seek.hip) and the batched GetRange merge (okv_pages.hip).
// Internal header.  Host mode of the batched calls -- the key check of an okv_rows, the layout
// of a staging buffer and the copies in and out of it -- is okv_stage.hpp, which a file
// includes after this one.
// Ownership: every device or pinned allocation is one DevBuf / PinBuf (okv_buf.hpp) that knows
// its capacity and frees itself with its owner; kernels get raw pointers from data().  The
// owners are okv_ctx (decode), AblateState (the decode ablation arms) and, each defined in its
// own file behind a forward declaration here and released by okv_close: EncScratch,
// zst::Scratch, mrg::Scratch, get::Scratch, snap::Scratch, zenc::Scratch, rng::Scratch and
// pages::Scratch.
#pragma once
#include <hip/hip_runtime.h>
#define OKV_BUF_HIP

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "okv_buf.hpp"
#include "okv_kernels.hpp"
#include "okv_sst.h"

namespace okv {
struct EncScratch;  // okv_encode.hip
void enc_release(okv_ctx* ctx);
namespace mrg {
struct Scratch;  // okv_merge.hip
}
void merge_release(okv_ctx* ctx);
namespace get {
struct Scratch;  // okv_get.hip
}
void get_release(okv_ctx* ctx);
namespace snap {
struct Scratch;  // okv_snap.hip
}
void snap_release(okv_ctx* ctx);
namespace rng {
struct Scratch;  // okv_seek.hip
}
void range_release(okv_ctx* ctx);
namespace pages {
struct Scratch;  // okv_pages.hip
}
void pages_release(okv_ctx* ctx);
// okv_bloom.hip: what another translation unit's kernel needs to probe a device filter.
struct BloomView {
  okv_ctx* ctx;
  const uint64_t* words;  // device, wordsNeeded(length) native words
  uint64_t m, k, length;
};
BloomView bloom_view(const okv_bloom* f);
// okv_decode.hip: enqueue XXH64 of each block's BlockSize bytes (device pointers).
void launch_hash(hipStream_t stream, const uint8_t* seg, uint64_t seg_bytes, const Desc* descs,
                 uint32_t nblk, uint64_t* out);
// okv_encode.hip: enqueue the one-workgroup exclusive scan of n u64 values (okv_enc_scan_kernel):
// out[i] = sum of in[j], j < i; *total (may be null) = the sum.  in and out are distinct.
void launch_scan_u64(hipStream_t stream, const uint64_t* in, uint64_t n, uint64_t* out,
                     unsigned long long* total);
// okv_zstd.hip: the zstd stage.  Every block of the batch (device pointers) is decompressed into
// the stage's own scratch; passes 1-3 then walk `bytes` by `descs` (offset into bytes,
// BlockSize = decompressed length), with `status` as each block's outcome so far.  The
// pointers hold until the context's next zstd decode.
namespace zst {
struct Scratch;  // okv_zstd.hip
}
struct ZstdOut {
  const uint8_t* bytes;
  uint64_t n_bytes;
  const Desc* descs;
  const int32_t* status;
  uint32_t retried;  // blocks that outgrew their first region and were decoded again
};
int zstd_stage(okv_ctx* ctx, const uint8_t* seg, uint64_t seg_bytes, const Desc* descs,
               uint32_t nblk, ZstdOut* out);
void zstd_release(okv_ctx* ctx);
// okv_zstd_enc.hip: the zstd encoder (OKV_F_ZSTD_NATIVE).  img_desc[b] (device) says where
// block b's raw records lie in the image: offset (16-byte aligned) and original_size.
// zstd_enc_bound computes the units and *bound_bytes, the data bytes when every block is
// stored as Raw_Blocks.  zstd_enc_run then compresses those blocks, writes the padded frames
// at DataBlockSize D into seg, the BlockStats over desc, their hashes into hash (device
// pointers) and the actual *data_bytes.  mode: what a unit's literals may become -- raw only,
// Huffman with direct weights where that is smaller (OKV_F_ZSTD_HUFFMAN), or Huffman over all
// byte values with direct or FSE-compressed weights (OKV_F_ZSTD_HUF_FSE).  *huffman_seen:
// bit 0, a unit of the call was written with Huffman literals; bit 1, one with FSE weights.
namespace zenc {
struct Scratch;  // okv_zstd_enc.hip
}
constexpr uint32_t kZencRaw = 0, kZencHuffman = 1, kZencFse = 2;
int zstd_enc_bound(okv_ctx* ctx, const Desc* img_desc, uint64_t nb, uint64_t D,
                   uint64_t* bound_bytes);
int zstd_enc_run(okv_ctx* ctx, const uint8_t* img, uint64_t img_bytes, Desc* desc, uint64_t nb,
                 uint64_t D, uint8_t* seg, uint64_t* hash, uint64_t* data_bytes, uint32_t mode,
                 uint32_t* huffman_seen);
void zstd_enc_release(okv_ctx* ctx);
}  // namespace okv

namespace okv {
// Knobs and scratch of the measured alternative decode arms.  Only the
// ablation build (-DOKV_ABLATE, okv_decode_ablate_host.inc) reads or writes
// it; in the product library it keeps these defaults and nothing looks at it.
struct AblateState {
  bool active = false;          // some knob below differs from the product form
  // knobs (okv_open reads them from the environment)
  bool group = false;           // OKV_DECODE_GROUP=1: grouped single pass (okv_group_kernel)
  bool pieces = false;          // OKV_DECODE_PIECES=1: large-block decodes in two pieces
  bool stream_lb = false;       // OKV_DECODE_STREAM=1: okv_decode_stream_kernel
  uint64_t small_piece = 0;     // OKV_SMALL_PIECE_MB: small-block decodes in pieces of these bytes
  uint32_t gather_grid = 0;     // 0: default grid; else workgroups (OKV_GATHER_GRID)
  uint32_t gather_threads = 0;  // 0: by average block size; else 64 or 256 (OKV_GATHER_THREADS)
  bool gather_staged = true;    // 256-thread pass 3 stages value spans in LDS (OKV_GATHER_STAGED=0: off)
  uint32_t value_sweep = 8;     // large blocks: 8 = okv_tile_kernel; 0 = the per-block staged
                                // pass 3; 1/2/4 (unaligned loads), 5/6/7 (aligned, 4/2/3) = rows +
                                // value sweep, tiles per workgroup; 9-11 = okv_block_kernel
  uint32_t tile_kib = 16;       // okv_tile_kernel tile bytes / 1024 (OKV_TILE)
  bool tile_xcd = true;         // consecutive tiles on one XCD
  uint32_t tile_threads = 256;  // okv_tile_kernel workgroup width
  uint32_t tile_diag = 0;       // diagnostic arms (1: no chunk pass, 2: no DMA, ...)
  // grouped single pass: look-back scratch
  DevBuf<uint32_t> g_flag;      // [groups] look-back flags, tagged with g_epoch (zeroed once)
  DevBuf<Prefix> g_agg;
  DevBuf<Prefix> g_incl;
  uint32_t g_epoch = 0;
  // decodes in pieces
  DevBuf<Totals> d_ptot;        // two Totals: the running prefix between small pieces
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_piece[2] = {nullptr, nullptr};
  DevBuf<Totals> d_tot2;        // totals of the first large piece
  // value sweep hand-off; the tile pass's phase probe uses d_vsrc too
  DevBuf<uint8_t> d_vsrc;       // [row] value sources
  DevBuf<uint32_t> d_vtile;     // [value-arena tile] owning rows
};
}  // namespace okv

struct okv_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  uint32_t last_path = 0;          // OKV_PATH_* of the last decode (okv_last_path)
  // open options
  bool fused = true;               // OKV_OPEN_NO_FUSED: passes 1-3 as separate launches
  uint32_t fused_max = 0;          // largest fused batch: resident-capacity bound (okv_open)
  bool zstd_one_pass = false;      // OKV_OPEN_ZSTD_ONE_PASS: every zstd block by the general kernel
  bool point = true;               // host-mode point path (okv_point_kernel); OKV_OPEN_NO_POINT: off
  // pass-1/2 scratch
  okv::DevBuf<okv::BlockCount> d_cnt;
  okv::DevBuf<okv::Prefix> d_lp;
  okv::DevBuf<okv::Prefix> d_tile_tot;
  okv::DevBuf<okv::Prefix> d_tile_pre;
  okv::DevBuf<uint32_t> d_rec;     // nblk x kRCap record positions (pass 1, rec_index)
  okv::DevBuf<uint32_t> d_big;     // big-block list [nblk]
  okv::DevBuf<uint32_t> d_ctr;     // zeroed once: [0] count-kernel arrivals, [1..2] big-block counters
  uint32_t big_slot = 0;           // slot the next launch counts big blocks in
  okv::DevBuf<uint16_t> d_hdr;     // [nblk x kRCap] pass-1 record key lengths: tile pass
  okv::DevBuf<okv::Totals> d_tot;
  okv::PinBuf<okv::Totals> h_tot;
  // the longest block walk of the last okv_decode_plan, for that batch's tile
  // pass (tile_geo); keyed by the batch's device inputs
  okv::DevBuf<unsigned long long> d_span;
  okv::PinBuf<unsigned long long> h_span;
  okv::SpanHint span_hint;
  // single-pass small-block decode (okv_decode_fused_kernel)
  okv::DevBuf<uint64_t> f_flag;    // [nblk] look-back words, tagged with f_epoch (zeroed once)
  okv::DevBuf<okv::Prefix> f_agg;
  okv::DevBuf<okv::Prefix> f_incl;
  okv::DevBuf<unsigned long long> f_ctr;  // zeroed once: block-index counter, f_base at the next call
  unsigned long long f_base = 0;        // (f_ctr, f_base: the ablation build's stream / block arms)
  uint32_t f_epoch = 0;
  // okv_decode_chain: this context's pass 3 waits for chain's last pass 3
  okv_ctx* chain = nullptr;
  std::vector<okv_ctx*> chained_by;  // contexts whose chain is this one (unchained at close)
  hipEvent_t p3_done = nullptr;    // recorded after every pass 3 once created
  bool p3_rec = false;             // p3_done has been recorded
  // host-mode staging buffers (device side)
  okv::DevBuf<uint8_t> d_seg;
  okv::DevBuf<okv::Desc> d_desc;
  okv::DevBuf<uint8_t> d_out;
  okv::DevBuf<uint64_t> d_hash;
  // host-mode point reads (okv_point_kernel): one pinned slab holding the
  // staged blocks, their descriptors and every output
  okv::PinBuf<uint8_t> h_slab;
  uint32_t point_seq = 0;          // point-kernel call number (its slab completion word)
  // per-pass event timing (okv_profile)
  bool prof = false;
  std::vector<hipEvent_t> ev;  // 5 per timed call
  size_t ev_used = 0;
  double prof_ms[4] = {0, 0, 0, 0};  // count, scan, gather, zstd stage
  uint64_t prof_calls = 0;
  okv::AblateState ab;             // the ablation build's arms (unused by the product)
  okv::EncScratch* enc = nullptr;  // encode scratch (okv_encode.hip)
  okv::mrg::Scratch* merge = nullptr;  // merge scratch (okv_merge.hip)
  okv::zst::Scratch* zstd = nullptr;   // zstd stage scratch (okv_zstd.hip)
  okv::get::Scratch* get = nullptr;    // batched GetRow scratch (okv_get.hip)
  okv::snap::Scratch* snap = nullptr;  // snapshot GetRows scratch (okv_snap.hip)
  okv::zenc::Scratch* zenc = nullptr;  // zstd encoder scratch (okv_zstd_enc.hip)
  okv::rng::Scratch* range = nullptr;  // seek and gather scratch (okv_seek.hip)
  okv::pages::Scratch* pages = nullptr;  // batched GetRange merge scratch (okv_pages.hip)
};

namespace okv {

// A/B and diagnostic knobs: read from the environment in the ablation build
// only (-DOKV_ABLATE, libokv_sst_ablate.so); the product library never reads
// the environment, so its kernels do not change with a process's settings.
inline const char* knob(const char* name) {
#ifdef OKV_ABLATE
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

inline int set_err(okv_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
  if (c) {
    c->err = what;
    if (e != hipSuccess) {
      c->err += ": ";
      c->err += hipGetErrorString(e);
    }
  }
  return code;
}

#define OKV_HIP(call)                                             \
  do {                                                            \
    hipError_t e_ = (call);                                       \
    if (e_ != hipSuccess) return set_err(ctx, OKV_E_HIP, #call, e_); \
  } while (0)

// The CUs of the context's device, what the grids are capped by (256 when the query fails).
inline uint32_t cu_count(okv_ctx* ctx) {
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device) !=
          hipSuccess || ncu <= 0)
    ncu = 256;
  return uint32_t(ncu);
}

// Room for n elements of scratch on the context's stream (Buf::reserve): a
// compare when there is room already; a failure is OKV_E_HIP with HIP's text.
template <class B>
inline int reserve(okv_ctx* ctx, B& b, size_t n, bool* fresh = nullptr) {
  const hipError_t e = b.reserve(ctx->stream, n, fresh);
  return e == hipSuccess ? OKV_OK : set_err(ctx, OKV_E_HIP, "scratch allocation", e);
}

}  // namespace okv
