/*
 * okv_sst.h -- C-ABI of the MI355X-native SST block decode path
 * (libokv_sst.so, objectkv_amd/csrc/).
 *
 * This is the drop-in boundary for ObjectKV's Go `sst` package
 * (danthegoodman1/ObjectKV @ 2025-03-21).  The reference has no FFI: its seam
 * is the Go method
 *     func (s *SegmentReader) ReadBlockWithStat(stat BlockStat) ([]KVPair, error)
 *     (sst/segment_reader.go:295-355)
 * called by RowIter.Next/Seek (sst/segment_row_iter.go:83, :143, :165),
 * GetRow (segment_reader.go:392) and GetRange (:458).  A cgo shim
 *  replaces that method's body -- and a batched
 * `ReadBlocks([]BlockStat)` used by RowIter and the compaction feed -- with
 * okv_decode_blocks() below.  Metadata parsing (FetchAndLoadMetadata,
 * BytesToMetadata, segment_reader.go:91-238) stays in the host caller; it
 * yields the okv_block_desc array.
 *
 * Plain pointers and sizes only.  All inputs and outputs are owned by the
 * caller; the library owns only its context (device, stream, scratch) and
 * retains no pointer after a call returns.  Contexts are not thread safe
 * (like the Go types, segment_writer.go:57): use one okv_ctx per (device,
 * goroutine/thread).
 */
#ifndef OKV_SST_H
#define OKV_SST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OKV_ABI_VERSION 6 /* 2: okv_encode_opts.bloom / bloom_len, and okv_profile_read writes
                             4 doubles (ms[4]: the zstd stage slot was added);
                             3: okv_open_ex / okv_open_opts
                             4: okv_decode_chain
                             5: OKV_OPEN_NO_POINT / OKV_PATH_POINT (host-mode point path)
                             6: okv_point_get (GetRow's block step, one row back);
                                still 6 with the device bloom filter (okv_bloom_*,
                                OKV_F_BLOOM_DEVICE): purely additive -- new symbols and one
                                new flag bit, no struct layout or behaviour change;
                                still 6 with the batched GetRow (okv_index_*, okv_get_*,
                                OKV_PATH_GET): new symbols only;
                                still 6 with the device zstd encoder (OKV_F_ZSTD_NATIVE,
                                OKV_PATH_ZSTD_ENC): one new flag bit and one path bit;
                                still 6 with the snapshot GetRows (okv_snap_*,
                                OKV_PATH_SNAP_GET): new symbols and one path bit;
                                still 6 with GetRows on zstd segments (OKV_F_GET_ZSTD,
                                OKV_GET_INFLATED_MAX): one new flag bit;
                                still 6 with Huffman literals in the device zstd encoder
                                (OKV_F_ZSTD_HUFFMAN, OKV_PATH_ZSTD_HUF): one new flag bit and
                                one path bit;
                                still 6 with FSE-compressed Huffman weights there
                                (OKV_F_ZSTD_HUF_FSE, OKV_PATH_ZSTD_HUF_FSE): one new flag bit
                                and one path bit;
                                still 6 with the range-split encode (okv_encode_split,
                                okv_split_*): new symbols only */

/* ---- return codes (int) -------------------------------------------------- */
#define OKV_OK 0
#define OKV_E_ARG (-1)      /* bad argument (NULL, misaligned device pointer, ...) */
#define OKV_E_HIP (-2)      /* HIP runtime failure; okv_last_error() has the text */
#define OKV_E_CAPACITY (-3) /* outputs too small: totals in okv_decode_out are set */
#define OKV_E_NOMEM (-4)
#define OKV_E_NODEV (-5)    /* no GPU / bad device id */

/* Go SegmentWriter sentinels returned by the encode (values shared with
 * okv_host.h and the test oracle; segment_writer.go:69-74) */
#define OKV_W_KEY_TOO_LARGE (-101)   /* ErrKeyTooLarge */
#define OKV_W_VALUE_TOO_LARGE (-102) /* ErrValueTooLarge */
#define OKV_W_CLOSED (-103)          /* ErrWriterClosed */
#define OKV_W_INVALID_KEY (-104)     /* ErrInvalidKey: empty key (WriteRow :89-91) */
#define OKV_W_NIL_WRITER (-105)      /* Go panics in Close when no block is open (:212, Q1) */
#define OKV_W_UNSUPPORTED (-106)     /* zstd level > 0 without OKV_F_ZSTD_NATIVE: the Go writer's
                                        bytes cannot be produced (Q6) */
#define OKV_W_NO_ROWS (-107)         /* ErrNoRowsWritten (:221-223) */

/* ---- per-block status (okv_decode_out.blk_status) ---------------------- */
/* Mirrors what ReadBlockWithStat does for that block (segment_reader.go). */
#define OKV_BLK_OK 0
#define OKV_BLK_EOF 1         /* Seek/Read error: offset >= segment length (:303-313) -> Go error */
#define OKV_BLK_SHORT 2       /* short read, ErrUnexpectedBytesRead (:314-316) -> Go error */
#define OKV_BLK_PANIC 3       /* record overruns the block buffer: mustReadBytes panics (:338-352, :506-512) */
#define OKV_BLK_UNSUPPORTED 4 /* zstd block under OKV_F_INDEX_ONLY (no spans into seg exist) */
#define OKV_BLK_CAPACITY 5    /* the caller's output capacity (row_cap / key_cap / val_cap) is
                                 exceeded (library-specific; never with okv_decode_plan sizes) */
#define OKV_BLK_ZSTD_ERROR 6  /* zstd.NewReader / io.Copy error (:321-330) -> Go error */

/* ---- compression byte of the meta block (segment_reader.go:166-172) ----- */
#define OKV_COMP_NONE 0
#define OKV_COMP_ZSTD 1 /* decoded on the device (okv_zstd.hip); not with OKV_F_INDEX_ONLY */
#define OKV_COMP_LZ4 2 /* reference quirk Q7: decodes as an empty buffer */

/* ---- flags ---------------------------------------------------------------- */
#define OKV_F_DEVICE_PTRS 1u /* seg, descs and every output pointer are device pointers */
#define OKV_F_INDEX_ONLY 2u  /* key_off/val_off are byte offsets into seg; no arenas written */
#define OKV_F_ASYNC 4u       /* with DEVICE_PTRS: enqueue on the ctx stream and return;
                                totals are NOT filled (call okv_decode_totals after okv_sync) */
#define OKV_F_NO_CLOSE 8u    /* encode: stop after blocks + block index + meta block; the
                                meta XXH64 and the 25-byte trailer are left to okv_encode_close */
#define OKV_F_BLOOM_DEVICE 16u /* okv_encode_rows: opts->bloom is a DEVICE pointer (copied device
                                to device on the ctx stream); independent of OKV_F_DEVICE_PTRS */
/* okv_encode_rows / okv_encode_close with opts->compression == OKV_COMP_ZSTD: the device zstd
 * encoder (okv_zstd_enc.hip).  Every block becomes one standard RFC 8878 frame
 * (Single_Segment, Frame_Content_Size = OriginalSize, Content_Checksum) that inflates to the
 * block's raw bytes; CompressedSize, the zero padding to DataBlockSize, Hash, Offset, the meta
 * block (compression byte 1) and the trailer are the Go writer's (segment_writer.go:148-204,
 * :284-328).  Opt-in, because two things differ from a Go writer with ZSTDCompressionLevel > 0:
 *  - the frame bytes are this encoder's, not klauspost/compress v1.17.9's;
 *  - a block is cut when its RAW length reaches threshold_bytes (the rule of
 *    oracle/zstd_ref.py zstd_segment); Go cuts on the klauspost encoder's buffered output
 *    length (Q6).  The row partition (blk_first_row, OriginalSize) is therefore the one the
 *    uncompressed encode gives for the same rows and threshold.
 * Without the flag OKV_COMP_ZSTD is OKV_W_UNSUPPORTED; the flag with any other compression is
 * OKV_E_ARG.
 * Capacity: compressed sizes exist only after the compress stage, so the sizes a call must
 * be given come from the raw sizes alone.  A call whose capacities are too small (the size
 * query included) sets n_blocks exactly and data_bytes / file_bytes to an upper bound -- every
 * block as Raw_Blocks plus frame overhead, padded -- writes nothing and returns
 * OKV_E_CAPACITY; a call with seg_cap >= that file_bytes and blk_cap >= n_blocks succeeds
 * and sets the actual sizes (never above the bound). */
#define OKV_F_ZSTD_NATIVE 64u
/* okv_get_rows / okv_snap_get_rows: take the floor blocks of OKV_COMP_ZSTD segments too
 * (DESIGN.md 25).  Without the flag such a block is OKV_GET_FALLBACK / OKV_SNAP_FALLBACK.
 * With it, for a segment whose compression is OKV_COMP_ZSTD (any other segment: no change):
 *  - the floor block is taken whatever its BlockSize.  Its status before any read is Go's
 *    in Go's order: :303-316 (EOF / PANIC / SHORT), then CompressedSize > BlockSize ->
 *    OKV_BLK_PANIC (the slice of :321);
 *  - every touched block is inflated once per call by the device decoder, its
 *    CompressedSize bytes only; a frame set the decoder rejects fails the block's keys with
 *    BLOCK_ERROR (SEG_ERROR) and blk_status = OKV_BLK_ZSTD_ERROR;
 *  - the record walk (:338-352, bounded by OriginalSize) runs over the whole inflated
 *    length, as Go inflates every frame before it; a failed walk is OKV_BLK_PANIC;
 *  - a block that inflates to more than OKV_GET_INFLATED_MAX bytes is FALLBACK for its
 *    keys (decided after the inflate);
 *  - FOUND: val_off is the value's offset INSIDE THE INFLATED BLOCK entry[i] names (there is
 *    no offset into seg); val_len and the bytes in val_arena are as ever.
 * The call synchronises with the host inside the call (the touched count and the zstd
 * stage's own round trips, as a zstd okv_decode_blocks does); OKV_F_ASYNC still defers only
 * the totals.  okv_last_path gains OKV_PATH_ZSTD when blocks were inflated, and
 * OKV_PATH_ZSTD_REGROW when some outgrew their first region. */
#define OKV_F_GET_ZSTD 128u
/* okv_encode_rows / okv_encode_close, only together with OKV_F_ZSTD_NATIVE (and so with
 * OKV_COMP_ZSTD); without OKV_F_ZSTD_NATIVE the call returns OKV_E_ARG.  The device zstd
 * encoder then writes a unit's literals as a Compressed_Literals_Block (RFC 8878 3.1.1.3.1:
 * Huffman-coded, the tree as direct 4-bit weights, code lengths at most 11, one stream up to
 * 1 023 literals and four above) where at least two byte values occur, none is above 128 and
 * the section is strictly smaller than the raw one; otherwise the literals stay raw and the
 * unit's bytes are those without the flag.  The sequences are the same as without the flag.
 * A unit without sequences may then be a Compressed_Block (its sequences section is the byte
 * 0).  Per unit the size is never above the size without the flag, so the capacity contract
 * and the bound of OKV_ZSTD_ENC_UNIT hold unchanged; without the flag every output byte is
 * what it was.  Opt-in; okv_last_path gains OKV_PATH_ZSTD_HUF when a unit was written so
 * (DESIGN.md 26). */
#define OKV_F_ZSTD_HUFFMAN 256u
/* okv_encode_rows / okv_encode_close, only together with OKV_F_ZSTD_HUFFMAN (and so with
 * OKV_F_ZSTD_NATIVE); otherwise the call returns OKV_E_ARG.  Literals with byte values above
 * 128 may then be Huffman-coded too: code lengths are computed over all 256 values, and the
 * tree is described by FSE-compressed weights (RFC 8878 4.2.1.2, accuracy log 5 or 6) where
 * that description exists and is strictly smaller than the direct one, or the direct one
 * cannot list the weights (a value above 128).  Per unit the size is never above the size
 * under OKV_F_ZSTD_HUFFMAN alone, so the capacity contract and the bound are unchanged;
 * without this flag every output byte is what it was.  Opt-in; okv_last_path gains
 * OKV_PATH_ZSTD_HUF_FSE when a unit was written so. */
#define OKV_F_ZSTD_HUF_FSE 512u
#define OKV_GET_INFLATED_MAX (1u << 24)
/* The most source bytes the encoder puts into one zstd block of a frame, so
 * CompressedSize <= OriginalSize + 3 * ceil(OriginalSize / OKV_ZSTD_ENC_UNIT) + 18. */
#define OKV_ZSTD_ENC_UNIT 32768

/* One data-block index entry: BlockStat (sst/block_stat.go:9-24) without
 * FirstKey and Hash, which the decode does not need. */
typedef struct okv_block_desc {
  uint64_t offset;          /* BlockStat.Offset         */
  uint64_t block_size;      /* BlockStat.BlockSize      */
  uint64_t original_size;   /* BlockStat.OriginalSize   */
  uint64_t compressed_size; /* BlockStat.CompressedSize */
} okv_block_desc;

/*
 * Output of a batched decode, structure-of-arrays (DESIGN.md "Output layout").
 * Global row g of block b is row (g - row_start[b]) of ReadBlockWithStat(b),
 * in block order (callers reverse per block for DirectionDescending,
 * segment_row_iter.go:89-92).  Per row:
 *   key bytes   = key_arena[key_off[g] .. +key_len[g]]   (full decode)
 *               = seg[key_off[g] .. +key_len[g]]         (OKV_F_INDEX_ONLY)
 *   value bytes = val_arena[val_off[g] .. +val_len[g]]   (likewise)
 *   a length of 0 is Go's nil slice (Q4: readBytes returns nil, :490-493).
 * In full-decode mode each block's keys (values) are packed contiguously at
 * key_base[b] (val_base[b]); each block region is zero-padded to a multiple
 * of 16 bytes, so key_base/val_base are 16-byte aligned.
 * A block whose status is not OKV_BLK_OK contributes no rows and no bytes.
 */
typedef struct okv_decode_out {
  uint64_t *row_start; /* [nblk+1] exclusive scan of rows per block  */
  uint64_t *key_base;  /* [nblk]   (full decode; may be NULL)          */
  uint64_t *val_base;  /* [nblk]   (full decode; may be NULL)          */
  int32_t *blk_status; /* [nblk]   OKV_BLK_*                           */
  uint64_t *key_off;   /* [row_cap] */
  uint16_t *key_len;   /* [row_cap] */
  uint64_t *val_off;   /* [row_cap] */
  uint32_t *val_len;   /* [row_cap] */
  uint8_t *key_arena;  /* [key_cap] (full decode) */
  uint8_t *val_arena;  /* [val_cap] (full decode) */
  uint64_t row_cap, key_cap, val_cap;
  /* filled on return (synchronous calls): */
  uint64_t n_rows;        /* total rows */
  uint64_t key_bytes;     /* arena extent used (sum of 16-byte padded block regions) */
  uint64_t val_bytes;     /* likewise for values */
  uint64_t n_bad_blocks;  /* blocks whose status != OKV_BLK_OK */
} okv_decode_out;

typedef struct okv_ctx okv_ctx;

/* Context bound to one GPU (HIP device ordinal).  Creates its own stream
 * unless okv_open_on_stream is used (stream = a hipStream_t, opaque here). */
okv_ctx *okv_open(int device);
okv_ctx *okv_open_on_stream(int device, void *stream);

/* Context options (okv_open_ex).  The library reads no environment variables:
 * every choice a caller can make is here. */
#define OKV_OPEN_NO_FUSED 1u      /* batches of <= 512 small blocks: three launches (count, scan,
                                     gather) instead of the single-pass kernel, whose workgroups
                                     wait for each other -- for devices whose compute slots other
                                     work may hold; the outputs are identical */
#define OKV_OPEN_ZSTD_ONE_PASS 2u /* zstd blocks: the one-wave-per-block decoder for every block
                                     (one launch, no host synchronisation between stages: lower
                                     latency for a few blocks); outputs identical */
#define OKV_OPEN_NO_POINT 4u      /* host-mode calls never take the point path (okv_point_kernel:
                                     <= 16 small uncompressed blocks in one launch over pinned
                                     memory): every batch is staged to device memory and decoded
                                     by the device-resident kernels; outputs identical */
typedef struct okv_open_opts {
  uint32_t size;  /* sizeof(okv_open_opts) */
  uint32_t flags; /* OKV_OPEN_* */
} okv_open_opts;
/* stream may be NULL (the context creates its own); opts may be NULL (defaults). */
okv_ctx *okv_open_ex(int device, void *stream, const okv_open_opts *opts);
void okv_close(okv_ctx *ctx);
const char *okv_last_error(const okv_ctx *ctx);
void *okv_stream(const okv_ctx *ctx);
int okv_sync(okv_ctx *ctx);
int okv_abi_version(void);

/*
 * Size query (pass 1 + scan only): totals needed by okv_decode_blocks for
 * these blocks.  Same inputs and flags as okv_decode_blocks (ASYNC ignored).
 */
int okv_decode_plan(okv_ctx *ctx, const uint8_t *seg, uint64_t seg_bytes,
                    const okv_block_desc *descs, uint32_t nblk, int compression,
                    uint32_t flags, uint64_t *n_rows, uint64_t *key_bytes,
                    uint64_t *val_bytes);

/*
 * Batched ReadBlockWithStat over `nblk` blocks of one segment.
 *   seg/seg_bytes : the segment file bytes (what the io.ReadSeeker holds).
 *                   Device pointers must be 16-byte aligned; the kernels issue
 *                   only aligned loads that contain at least one byte of
 *                   [seg, seg+seg_bytes).
 *   compression   : the meta block's compression byte (OKV_COMP_*).
 * Returns OKV_OK, OKV_E_CAPACITY (totals set; nothing else is valid), or a
 * negative error.  Per-block outcomes are in out->blk_status.
 */
int okv_decode_blocks(okv_ctx *ctx, const uint8_t *seg, uint64_t seg_bytes,
                      const okv_block_desc *descs, uint32_t nblk, int compression,
                      okv_decode_out *out, uint32_t flags);

/*
 * Consecutive-segment pipelining (a reader decoding segment after segment: a
 * compaction feed, a scan over a level).  After okv_decode_chain(ctx, after),
 * every decode on ctx starts its pass 3 (the bandwidth-bound kernels) only
 * once the pass 3 last enqueued on `after` has finished.  Two contexts chained
 * to each other, decoding alternate segments on their own streams, run each
 * decode's header walk (pass 1, latency-bound) under the other's pass 3,
 * while their pass-3 kernels never run concurrently.  after = NULL unchains.
 * Both contexts must be on the same device and be driven from one host thread;
 * okv_close of either unchains the pair.  The caller's current device is kept.
 */
int okv_decode_chain(okv_ctx *ctx, okv_ctx *after);

/*
 * GetRow's block step (segment_reader.go:387-404) on one block, host memory:
 * ReadBlockWithStat of the block -- every record walked with Go's checks --
 * then the first row whose key equals `key` (bytes.Equal, :398), in one
 * point-path launch (okv_point_kernel: the block and the key in, that one
 * row out; no row arrays come back).
 *   out->status : the block's OKV_BLK_* outcome (rows exist only when OK);
 *   out->found  : 1 (key / val point at the row's bytes, valid until the next
 *                 call on ctx), 0 (no such row), or -1 (the block is not a
 *                 point-path block -- zstd, BlockSize > 64 KiB, a key longer
 *                 than 8 KiB, or more than 1 024 rows: use okv_decode_blocks).
 * Returns OKV_OK or a negative error.  (ABI 6.)
 */
typedef struct okv_point_row {
  int32_t status;
  int32_t found;
  const uint8_t *key;
  uint64_t key_len;
  const uint8_t *val;
  uint64_t val_len;
} okv_point_row;

int okv_point_get(okv_ctx *ctx, const uint8_t *seg, uint64_t seg_bytes,
                  const okv_block_desc *desc, int compression, const uint8_t *key,
                  uint64_t key_len, okv_point_row *out);

/* After an OKV_F_ASYNC decode and okv_sync(): copy the device totals into out. */
int okv_decode_totals(okv_ctx *ctx, okv_decode_out *out);

/* XXH64 (cespare/xxhash/v2 v2.2.0 semantics, seed 0 in the reference) of a
 * host buffer. */
uint64_t okv_xxh64(const void *data, size_t len, uint64_t seed);

/* Device XXH64 of each block's BlockSize bytes at its Offset -- the value the
 * writer stored in BlockStat.Hash (segment_writer.go:185).  hashes[nblk]. */
int okv_hash_blocks(okv_ctx *ctx, const uint8_t *seg, uint64_t seg_bytes,
                    const okv_block_desc *descs, uint32_t nblk, uint64_t *hashes,
                    uint32_t flags);

/* ======================================================================== *
 * Encode: SegmentWriter.WriteRow x n -> Close (segment_writer.go:80-328)
 * ======================================================================== */

/* Rows to encode, structure of arrays (the okv_decode_out layout, so a decode
 * feeds an encode directly -- the compaction shape).  Row i is
 *   key   = key_arena[key_off[i] .. +key_len[i]]
 *   value = val_arena[val_off[i] .. +val_len[i]]
 * in the order WriteRow would be called ("expected that rows are written in
 * order", segment_writer.go:78; the writer does not check it and neither do
 * we).  key_arena_bytes / val_arena_bytes are the arena extents (host mode
 * stages that many bytes; device mode uses them only for validation). */
typedef struct okv_rows {
  const uint8_t *key_arena;
  const uint64_t *key_off;
  const uint16_t *key_len;
  const uint8_t *val_arena;
  const uint64_t *val_off;
  const uint32_t *val_len;
  uint64_t n_rows;
  uint64_t key_arena_bytes, val_arena_bytes;
} okv_rows;

/* SegmentWriterOptions (segment_writer_option.go:5-16).  The encoder treats the
 * bloom filter as opaque bytes: BloomFilter.WriteTo's output after Add has run
 * for every row (segment_writer.go:133-136), either from the caller's host
 * filter or, with OKV_F_BLOOM_DEVICE, from okv_bloom_add_rows +
 * okv_bloom_write_to on the device; the meta block then carries
 * [1][u64 LE length][bytes] (:295-300), else [0]. */
typedef struct okv_encode_opts {
  uint64_t threshold_bytes; /* DataBlockThresholdBytes (default 3584) */
  uint64_t block_size;      /* DataBlockSize (default 4096) */
  int compression;          /* OKV_COMP_NONE, or OKV_COMP_LZ4: Go writes raw bytes with
                               CompressedSize = OriginalSize and meta byte 2 (Q7);
                               OKV_COMP_ZSTD: with OKV_F_ZSTD_NATIVE the device encoder,
                               else OKV_W_UNSUPPORTED */
  int strict_go;            /* 1: a Close with no open block panics in Go (Q1) ->
                               OKV_W_NIL_WRITER; 0: write the footer normally */
  const uint8_t *bloom;     /* bytes of BloomFilter.WriteTo (host memory; device memory with
                               OKV_F_BLOOM_DEVICE), or NULL (BloomFilter nil) */
  uint64_t bloom_len;
} okv_encode_opts;

/* Output: the segment file, written as the Go writer writes it:
 *   seg[0 .. data_bytes)                      data blocks (BlockStat order)
 *   seg[data_bytes .. +meta_bytes)            meta block (generateMetaBlock :284-328)
 *   seg[data_bytes + meta_bytes .. +25)       trailer: u64 meta offset, u64 XXH64(meta),
 *                                             u8 version 1, u64 magic (:226-276)
 * plus the block index as arrays.  Any of blk_first_row / blk_desc / blk_hash
 * may be NULL.  FirstKey of block b = key of row blk_first_row[b]. */
typedef struct okv_encode_out {
  uint8_t *seg;
  uint64_t seg_cap;
  uint64_t *blk_first_row;  /* [blk_cap + 1]; entry n_blocks = n_rows */
  okv_block_desc *blk_desc; /* [blk_cap] Offset, BlockSize, OriginalSize, CompressedSize */
  uint64_t *blk_hash;       /* [blk_cap] BlockStat.Hash */
  uint64_t blk_cap;
  /* filled on return (also with OKV_E_CAPACITY): */
  uint64_t n_blocks;
  uint64_t data_bytes;  /* sum of BlockSize == meta block offset */
  uint64_t meta_bytes;
  uint64_t file_bytes;  /* data + meta + 25: Close()'s first return value */
  uint64_t meta_hash;   /* 0 with OKV_F_NO_CLOSE until okv_encode_close */
  uint64_t bad_row;     /* OKV_W_INVALID_KEY: the first row with an empty key */
} okv_encode_out;

/*
 * Encode rows into one segment on the GPU.  flags: OKV_F_DEVICE_PTRS (rows and
 * every output pointer are device pointers; seg should be 16-byte aligned: a seg that is
 * not is accepted and written by the slower byte-store pack kernels, same bytes),
 * OKV_F_NO_CLOSE, OKV_F_BLOOM_DEVICE, OKV_F_ZSTD_NATIVE, OKV_F_ZSTD_HUFFMAN (with
 * OKV_F_ZSTD_NATIVE only), OKV_F_ZSTD_HUF_FSE (with OKV_F_ZSTD_HUFFMAN only).  Returns OKV_OK; OKV_E_CAPACITY (sizes in out set, nothing
 * written: call again with seg_cap >= file_bytes and blk_cap >= n_blocks --
 * a call with zero capacities is the size query); OKV_W_INVALID_KEY (bad_row
 * set); OKV_W_NIL_WRITER (strict_go and the last row closed a block, or no
 * rows); OKV_W_NO_ROWS (no rows, strict_go == 0); OKV_W_UNSUPPORTED; or an
 * OKV_E_* error.
 */
int okv_encode_rows(okv_ctx *ctx, const okv_rows *rows, const okv_encode_opts *opts,
                    okv_encode_out *out, uint32_t flags);

/* Close after OKV_F_NO_CLOSE: XXH64 of the meta block on the host (one
 * sequential hash, segment_writer.go:248) and the trailer written into seg.
 * flags: OKV_F_DEVICE_PTRS as given to okv_encode_rows. */
int okv_encode_close(okv_ctx *ctx, okv_encode_out *out, uint32_t flags);

/* ---- range-split encode ---------------------------------------------------
 * A compaction's output segments from one call (sst/COMPACTION.md: "Ranges should be split by
 * size at compaction time"; sst/compaction_range.go: rangeSplitThresholdBytes 1_000_000,
 * rangeSplitThresholdRows 100_000).  The rows are cut into blocks exactly as okv_encode_rows
 * cuts them (one greedy chain over the whole row list); a segment is a run of consecutive
 * blocks of that chain.  The segment starting at block i ends with the first block j >= i for
 * which sum BlockSize[i..j] >= split_bytes (split_bytes != 0) or rows(i..j) >= split_rows
 * (split_rows != 0); if neither holds before the last block it ends with the last block.  Both
 * zero: one segment.  This is what a Go caller gets by watching the writer's flushed bytes and
 * rows after each WriteRow and closing right after a flush.  Closing right after a flush is
 * reference quirk Q1 (Go's Close panics on a nil block writer), so the call has strict_go == 0
 * semantics only: opts->strict_go != 0 is OKV_E_ARG. */
typedef struct okv_split_opts {
  uint64_t split_bytes, split_rows; /* 0: no limit */
  uint64_t bloom_m, bloom_k;        /* bloom_k == 0: BloomFilter nil; else one bloom.New(m, k)
                                       per segment (max(1, m), max(1, k) as Go), Add for each of
                                       its keys; bloom_k > 4096: OKV_E_ARG */
} okv_split_opts;

typedef struct okv_split_seg { /* one output segment */
  uint64_t first_row, n_rows, first_block, n_blocks;
  uint64_t data_off, data_bytes; /* into out->data */
  uint64_t meta_off, meta_bytes; /* into out->meta; the 25-byte trailer follows the meta block */
  uint64_t meta_hash, file_bytes; /* file = data span ++ meta span ++ trailer */
} okv_split_seg;

/* File s is data[data_off, +data_bytes) ++ meta[meta_off, +meta_bytes + 25): two spans, ready
 * for a vectored write or a multipart upload.  The data blocks of all segments, end to end,
 * are byte for byte okv_encode_rows' data blocks of the same rows. */
typedef struct okv_split_out {
  uint8_t *data;            /* every data block, in row order */
  uint64_t data_cap;
  uint8_t *meta;            /* per segment its meta block and trailer, at 16-byte-aligned
                               meta_off (a device meta must be 16-byte aligned itself) */
  uint64_t meta_cap;
  okv_split_seg *segs;      /* [seg_cap] */
  uint64_t seg_cap;
  uint64_t *blk_first_row;  /* [blk_cap + 1], optional, as in okv_encode_out */
  okv_block_desc *blk_desc; /* [blk_cap], optional; Offset is relative to the block's segment */
  uint64_t *blk_hash;       /* [blk_cap], optional */
  uint64_t blk_cap;
  /* filled on return (also with OKV_E_CAPACITY): */
  uint64_t n_segments;
  uint64_t n_blocks;
  uint64_t data_bytes;
  uint64_t meta_arena_bytes; /* sum over segments of round16(meta_bytes + 25) */
  uint64_t bad_row;          /* OKV_W_INVALID_KEY: the first row with an empty key */
} okv_split_out;

/*
 * flags: OKV_F_DEVICE_PTRS (rows and every output pointer are device pointers; meta must be
 * 16-byte aligned, else OKV_E_ARG; data should be, as seg of okv_encode_rows) or none (host
 * memory, staged); OKV_F_ZSTD_* and OKV_F_NO_CLOSE are
 * OKV_E_ARG.  opts->bloom must be NULL (the filters are the call's own), opts->compression
 * OKV_COMP_NONE or OKV_COMP_LZ4 (Q7).  Returns OKV_OK; OKV_E_CAPACITY (the sizes in out set,
 * nothing written: a call with zero capacities is the size query; a following call needs
 * data_cap >= data_bytes, meta_cap >= meta_arena_bytes, seg_cap >= n_segments and, with any
 * blk_* array, blk_cap >= n_blocks); OKV_W_INVALID_KEY (bad_row set); OKV_W_NO_ROWS; row
 * limits and validation as okv_encode_rows.  Every meta hash and trailer is computed on the
 * device; the number of host synchronisations does not depend on the number of segments.
 */
int okv_encode_split(okv_ctx *ctx, const okv_rows *rows, const okv_encode_opts *opts,
                     const okv_split_opts *split, okv_split_out *out, uint32_t flags);

/* Per-phase encode timing (HIP events on the ctx stream, enabled by
 * okv_profile(ctx, 1)): ms[4] = cut (E1-E9), pack, block hash, meta block,
 * summed over the profiled okv_encode_rows calls. */
int okv_encode_profile_read(okv_ctx *ctx, double *ms, uint64_t *calls);
int okv_encode_profile_reset(okv_ctx *ctx);

/* Deterministic C1/C2/C4 rows on the device: key = row index big-endian in
 * key_len bytes, value = val_len bytes of splitmix64(seed) 8-byte LE words,
 * drawn in row order (oracle/pyoracle.py rows_fixed).  Rows first_row ..
 * first_row + n - 1, packed: key_off[i] = i * key_len, val_off[i] = i * val_len
 * (relative to this call's arenas).  All pointers are device pointers. */
int okv_synth_rows_fixed(okv_ctx *ctx, uint64_t seed, uint64_t first_row, uint64_t n,
                         uint32_t key_len, uint32_t val_len, uint8_t *key_arena,
                         uint64_t *key_off, uint16_t *key_len_out, uint8_t *val_arena,
                         uint64_t *val_off, uint32_t *val_len_out);

/* ======================================================================== *
 * Bloom filter on the device: bloom.BloomFilter (bits-and-blooms v2.0.3 over
 * murmur3 v1.1.0 and bitset v1.1.11), the filter DefaultSegmentWriterOptions
 * carries (segment_writer_option.go:20).  WriteRow's Add per row
 * (segment_writer.go:133-136) becomes okv_bloom_add_rows over rows in device
 * memory, generateMetaBlock's WriteTo (:295-300) okv_bloom_write_to, and the
 * bytes go to okv_encode_rows with OKV_F_BLOOM_DEVICE: in stream order, with no
 * host copy of keys or filter.  Bytes equal Go's WriteTo (PARITY UNPINNED as in
 * okv_host.cpp: no reference test asserts filter bytes).  DESIGN.md 19.
 *
 * flags: OKV_F_DEVICE_PTRS (the arrays of okv_rows, `maybe` and `dst` are device
 * pointers) and OKV_F_ASYNC (with DEVICE_PTRS: enqueue on the ctx stream and
 * return); host mode stages the key arrays, runs and synchronises.  Of okv_rows
 * only key_arena, key_off, key_len, n_rows and key_arena_bytes are read (the
 * value fields may be NULL); empty keys are legal (Add accepts them);
 * n_rows == 0 succeeds and launches nothing.  The kernels read a key as aligned
 * 8-byte words that each contain at least one byte of it.
 * A filter belongs to the context that created it (another one: OKV_E_ARG) and
 * must be freed before that context is closed.
 *
 * Divergences from Go, all OKV_E_ARG: k > 4096 on add and test (Go has no cap;
 * a ReadFrom header must not size an unbounded loop); add on a filter whose
 * bitset length != m (Go's bitset.Set would grow the set); test with m == 0
 * and k > 0 (Go's integer-division panic; the host probe: OKV_R_PANIC).
 * ======================================================================== */
typedef struct okv_bloom okv_bloom; /* bloom.BloomFilter resident on the device */
#define OKV_BLOOM_FORCE_LDS 32u    /* okv_bloom_add_rows: the LDS-sliced form (filters of up to
                                      1 MiB of words; larger: OKV_E_ARG) */
#define OKV_BLOOM_FORCE_GLOBAL 64u /* okv_bloom_add_rows: one global atomic OR per location */
#define OKV_BLOOM_PATH_LDS 1u      /* okv_bloom_add_lds_kernel */
#define OKV_BLOOM_PATH_GLOBAL 2u   /* okv_bloom_add_global_kernel */

/* bloom.EstimateParameters(n, p); host only, no context */
void okv_bloom_estimate(uint64_t n, double p, uint64_t *m, uint64_t *k);
/* bloom.New: max(1, m), max(1, k), bitset length = m, every bit zero */
int okv_bloom_new(okv_ctx *ctx, uint64_t m, uint64_t k, okv_bloom **out);
/* BloomFilter.ReadFrom of host bytes (big-endian m, k, bitset length, words): a
 * short input or too few words is OKV_E_ARG and no object; trailing bytes are
 * ignored */
int okv_bloom_read_from(okv_ctx *ctx, const uint8_t *host_bytes, uint64_t len, okv_bloom **out);
void okv_bloom_free(okv_bloom *f);
/* write_to_bytes = 24 + 8 * wordsNeeded(length); any output pointer may be NULL */
int okv_bloom_info(const okv_bloom *f, uint64_t *m, uint64_t *k, uint64_t *length,
                   uint64_t *write_to_bytes);
/* ClearAll (enqueued on the ctx stream) */
int okv_bloom_clear(okv_ctx *ctx, okv_bloom *f);
/* Add(key) for every row.  flags also takes OKV_BLOOM_FORCE_LDS / _GLOBAL */
int okv_bloom_add_rows(okv_ctx *ctx, okv_bloom *f, const okv_rows *rows, uint32_t flags);
/* Test(key) for every row: maybe[i] = 1 (maybe present) or 0 (absent); k == 0
 * gives 1 for every key */
int okv_bloom_test_rows(okv_ctx *ctx, const okv_bloom *f, const okv_rows *rows, uint8_t *maybe,
                        uint32_t flags);
/* WriteTo: write_to_bytes bytes into dst (a device dst must be 8-byte aligned:
 * else OKV_E_ARG); cap too small: OKV_E_CAPACITY */
int okv_bloom_write_to(okv_ctx *ctx, const okv_bloom *f, uint8_t *dst, uint64_t cap,
                       uint32_t flags);
/* The form the filter's last okv_bloom_add_rows took (OKV_BLOOM_PATH_*; 0: it
 * launched nothing), in the manner of okv_last_path */
uint32_t okv_bloom_last_path(const okv_bloom *f);

/* ======================================================================== *
 * Batched GetRow: SegmentReader.GetRow (segment_reader.go:362-404) for many keys
 * against one segment in device memory, in one call.  Per key, in Go's order:
 * the bloom probe (:371-378; a rejected key touches no block, even a corrupt
 * one), DescendLessOrEqual over the block index for the floor block (:381-389),
 * ReadBlockWithStat of that block in full (:392; a block whose walk fails fails
 * the key even when an equal key sits before the bad record), then the first row
 * with bytes.Equal(row.Key, key) (:395-403; nil equals empty).  Keys are grouped
 * by floor block on the device, so a block is read once per call however many
 * keys land on it.  DESIGN.md 20.
 *
 * okv_index is SegmentMetadata.BlockIndex on the device: google/btree built by
 * ReplaceOrInsert in meta-block order, so of entries with an equal FirstKey the
 * last one stays (Q9).  n_tree counts the entries that stayed, n_file those given.
 * ======================================================================== */
typedef struct okv_index okv_index;
/* host pointers, meta-block order: entry i has descs[i] and the first key
 * fk_arena[fk_off[i] .. +fk_len[i]]; n_entries == 0 is legal (every key: no block) */
int okv_index_new(okv_ctx *ctx, const okv_block_desc *descs, const uint8_t *fk_arena,
                  const uint64_t *fk_off, const uint16_t *fk_len, uint64_t n_entries,
                  okv_index **out);
void okv_index_free(okv_index *ix);
int okv_index_info(const okv_index *ix, uint64_t *n_tree, uint64_t *n_file);

#define OKV_GET_FOUND 0
#define OKV_GET_BLOOM_NEGATIVE 1 /* ErrNoRows, "did not find row in bloom filter" (:371-378) */
#define OKV_GET_NO_BLOCK 2       /* ErrNoRows, no index entry <= key (:387-389) */
#define OKV_GET_NOT_IN_BLOCK 3   /* ErrNoRows, "did not find row in block" (:403) */
#define OKV_GET_BLOCK_ERROR 4    /* blk_status[i] = OKV_BLK_EOF / _SHORT / _PANIC (with
                                    OKV_F_GET_ZSTD also OKV_BLK_ZSTD_ERROR) */
#define OKV_GET_FALLBACK 5       /* not a block this path takes (zstd without OKV_F_GET_ZSTD or
                                    inflating past OKV_GET_INFLATED_MAX; uncompressed
                                    BlockSize > 64 KiB): use okv_decode_blocks */

typedef struct okv_get_out {
  int32_t *state;      /* [n] OKV_GET_* */
  int32_t *blk_status; /* [n] OKV_BLK_* of the floor block (OKV_BLK_OK when none was read) */
  uint32_t *entry;     /* [n] file index of the floor block, UINT32_MAX when none */
  uint64_t *val_off;   /* [n] FOUND: byte offset of the value in seg (else 0); in a zstd
                          segment (OKV_F_GET_ZSTD): inside the inflated block entry[i] */
  uint32_t *val_len;   /* [n] FOUND: its length, 0 <=> nil (else 0) */
  uint64_t *val_pos;   /* [n] or NULL: offset of the value in val_arena, 16-byte aligned;
                          keys that are not FOUND take no room */
  uint8_t *val_arena;  /* or NULL (index only); each value is zero-padded to 16 bytes;
                          a device arena must be 16-byte aligned */
  uint64_t val_cap;
  /* filled on return (also with OKV_E_CAPACITY, then val_arena is not written): */
  uint64_t n_found, n_fallback, val_bytes, blocks_searched;
} okv_get_out;

/*
 * seg is device memory (16-byte aligned); the kernels read inside round16(seg_bytes).
 * keys: of okv_rows only key_arena, key_off, key_len, n_rows and key_arena_bytes are
 * read; fewer than 2^32 keys.  bloom may be NULL (no filter: no probe).  The index and
 * the filter belong to ctx (another context: OKV_E_ARG).  A filter with m == 0 and
 * k > 0, or k > 4096, is OKV_E_ARG (okv_bloom_test_rows' divergences).
 * flags: without OKV_F_DEVICE_PTRS the key arrays and every output are host memory
 * (staged; the call synchronises); with it, optionally OKV_F_ASYNC, everything stays
 * in stream order (totals then by okv_get_totals after okv_sync).  n_rows == 0
 * succeeds and launches nothing.  OKV_F_GET_ZSTD: see the flag.
 * Returns OKV_OK, OKV_E_CAPACITY (val_bytes > val_cap:
 * totals and the per-key arrays are set, val_arena is not written), or an error.
 */
int okv_get_rows(okv_ctx *ctx, const uint8_t *seg, uint64_t seg_bytes, const okv_index *ix,
                 const okv_bloom *bloom, const okv_rows *keys, int compression,
                 okv_get_out *out, uint32_t flags);
/* After an OKV_F_ASYNC okv_get_rows and okv_sync(): the totals of the context's last call
 * (OKV_E_CAPACITY as the synchronous call would have returned it). */
int okv_get_totals(okv_ctx *ctx, okv_get_out *out);

/* ======================================================================== *
 * Snapshot GetRows: snapshot_reader.Reader.GetRow (snapshot_reader.go:104-149)
 * for many keys against the segments of a snapshot, in one call.  Per key, in
 * Go's order: the candidate segments (getPossibleSegmentsForKey, :152-171:
 * DescendLessOrEqual over blockRangeTree from {FirstKey: key}, collecting while
 * FirstKey <= key <= LastKey and stopping at the first record that fails, so a
 * segment below a non-covering one is never asked); the candidates by Level
 * ascending, then ID descending (:109-116); SegmentReader.GetRow of each in
 * turn as okv_get_rows states it -- ErrNoRows moves on, a block error ends the
 * key, a found row answers, and an empty value found at level 0 is a delete
 * (:136-141).  A candidate after the one that answers is never consulted: the
 * device probes every candidate (speculatively) and hides those outcomes.
 * DESIGN.md 22.
 *
 * okv_snap is blockRangeTree on the device.  segs come in tree order
 * (blockRangeLessFunc, :28-60: the host computes it) and `priority` is the
 * segment's rank in GetRow's order: 0 is asked first; the priorities of a
 * snapshot are a permutation of 0 .. n_segs - 1 (else OKV_E_ARG).  The snapshot
 * keeps the pointers it is given: it owns neither the segments' bytes nor their
 * indexes nor their filters, which must all outlive it and belong to ctx.
 * ======================================================================== */
typedef struct okv_snap okv_snap;
typedef struct okv_snap_seg {
  const uint8_t *seg;      /* device memory, 16-byte aligned; reads stay inside round16(seg_bytes) */
  uint64_t seg_bytes;
  const okv_index *index;  /* of ctx (another context: OKV_E_ARG) */
  const okv_bloom *bloom;  /* of ctx, or NULL: no probe.  m == 0 with k > 0, or k > 4096:
                              OKV_E_ARG, as okv_get_rows */
  const uint8_t *first_key; /* host bytes: SegmentRecord.Metadata.FirstKey / LastKey */
  const uint8_t *last_key;
  uint16_t first_len, last_len;
  int32_t compression;     /* OKV_COMP_* */
  uint32_t level;
  uint32_t priority;
} okv_snap_seg;
/* n_segs == 0 is legal (every key: OKV_SNAP_NO_ROWS); fewer than 2^32 - 1 blocks in all */
int okv_snap_new(okv_ctx *ctx, const okv_snap_seg *segs, uint32_t n_segs, okv_snap **out);
void okv_snap_free(okv_snap *snap);

#define OKV_SNAP_FOUND 0     /* val_off / val_len (0 <=> nil) in segment `seg` */
#define OKV_SNAP_NO_ROWS 1   /* ErrNoRows: no candidate has the row */
#define OKV_SNAP_DELETED 2   /* ErrNoRows too: an empty value found at level 0 (:136-141) */
#define OKV_SNAP_SEG_ERROR 3 /* blk_status[i] = OKV_BLK_EOF / _SHORT / _PANIC of segment `seg`
                                (with OKV_F_GET_ZSTD also OKV_BLK_ZSTD_ERROR) */
#define OKV_SNAP_FALLBACK 4  /* the resolution reached, before any answer, a candidate this path
                                does not take (zstd without OKV_F_GET_ZSTD or inflating past
                                OKV_GET_INFLATED_MAX; uncompressed BlockSize > 64 KiB): send the
                                whole key through the single-key path */

typedef struct okv_snap_out {
  int32_t *state;      /* [n] OKV_SNAP_* */
  uint32_t *seg;       /* [n] the answering (FOUND, DELETED) or failing (SEG_ERROR, FALLBACK)
                          segment's position in segs as given; UINT32_MAX when none */
  int32_t *blk_status; /* [n] OKV_BLK_* of that segment's floor block (OKV_BLK_OK otherwise) */
  uint32_t *entry;     /* [n] file index of that floor block, UINT32_MAX when none */
  uint64_t *val_off;   /* [n] FOUND: byte offset of the value in that segment (else 0); in a
                          zstd segment (OKV_F_GET_ZSTD): inside the inflated block entry[i] */
  uint32_t *val_len;   /* [n] FOUND: its length, 0 <=> nil (else 0) */
  uint64_t *val_pos;   /* [n] or NULL: offset of the value in val_arena, 16-byte aligned;
                          keys that are not FOUND take no room */
  uint8_t *val_arena;  /* or NULL (index only); each value is zero-padded to 16 bytes;
                          a device arena must be 16-byte aligned */
  uint64_t val_cap;
  /* filled on return (also with OKV_E_CAPACITY, then val_arena is not written): */
  uint64_t n_found, n_deleted, n_fallback, val_bytes;
  uint64_t pairs_probed;    /* (key, candidate segment) pairs: every candidate is probed */
  uint64_t blocks_searched; /* distinct (segment, floor block) staged and walked, once each */
} okv_snap_out;

/*
 * keys, flags (OKV_F_GET_ZSTD included: a snapshot may mix segment kinds), n_rows == 0 and
 * OKV_E_CAPACITY as okv_get_rows.  Fewer than 2^32 keys,
 * and n_rows * n_segs < 2^32 (the pair scratch is sized for every key meeting every
 * segment; more: OKV_E_ARG).  There is no cap on the candidates of one key.
 */
int okv_snap_get_rows(okv_ctx *ctx, const okv_snap *snap, const okv_rows *keys,
                      okv_snap_out *out, uint32_t flags);
/* After an OKV_F_ASYNC okv_snap_get_rows and okv_sync(): the totals of the context's last
 * call (OKV_E_CAPACITY as the synchronous call would have returned it). */
int okv_snap_totals(okv_ctx *ctx, okv_snap_out *out);

/* ======================================================================== *
 * Merge: snapshot_reader.Reader.GetRange's k-way merge
 * (/root/reference/snapshot_reader/snapshot_reader.go:214-372) on the device,
 * and the same newest-wins merge as a compaction feed.
 * ======================================================================== */
#define OKV_MERGE_GETRANGE 0 /* the Go loop exactly: range bound, limit, tombstones, and the
                                stale cursor of a stream that ran out (:336-365) */
#define OKV_MERGE_ALL 1      /* every key's owning row (compaction); L0 tombstones dropped
                                iff drop_tombstones */
#define OKV_DIR_ASC 0        /* sst.DirectionAscending  (segment_row_iter.go:22-25) */
#define OKV_DIR_DESC 1       /* sst.DirectionDescending */
#define OKV_M_EOF 1          /* okv_merge_out.status: GetRange returns an error because a
                                RowIter.Next hit io.EOF rolling a tombstone forward (:316-331) */

/* One merge input: rows [row_lo, row_hi) of a decoded segment (the okv_decode_out
 * layout, device pointers), sorted ascending by key as the Go writer writes them.
 * For GetRange this is the stream RowIter(direction).Seek(startRange) yields
 * (ascending: rows >= start; descending: rows <= end, consumed from row_hi - 1).
 * Inputs are given in the snapshot's priority order (:235-254); among equal keys
 * the lowest index owns the key (findMaxIndexes, :404-424).
 *
 * What the callee relies on and the tests pin (tests/test_merge_gpu.py):
 *  - an input with row_lo == row_hi is ignored: it owns nothing and, in
 *    OKV_MERGE_GETRANGE, takes no part in the loop (Go fails before the loop on a
 *    segment without a first row: the caller's check);
 *  - the rows [row_lo, row_hi) of each input must be strictly ascending by key
 *    (bytes.Compare, keys of up to 65535 bytes); unsorted or repeated keys inside one
 *    input give unspecified rows;
 *  - OKV_MERGE_GETRANGE assumes non-empty keys, as the writer guarantees
 *    (segment_writer.go:90-91): Go's `lastKey != ""` test makes the loop treat an empty
 *    key differently.  OKV_MERGE_ALL orders the empty key first like any other. */
typedef struct okv_merge_src {
  const uint8_t *key_arena;
  const uint64_t *key_off;
  const uint16_t *key_len;
  const uint8_t *val_arena;
  const uint64_t *val_off;
  const uint32_t *val_len; /* 0 = Go nil: an L0 row with a nil value is a tombstone */
  uint64_t row_lo, row_hi;
  int32_t level; /* SegmentRecord.Level */
  int32_t pad;
} okv_merge_src;

typedef struct okv_merge_opts {
  int mode;            /* OKV_MERGE_* */
  int direction;       /* OKV_DIR_* */
  int drop_tombstones; /* OKV_MERGE_ALL only */
  int pad;
  uint64_t limit;      /* OKV_MERGE_GETRANGE: > 0 (Go panics on 0: the caller's check) */
  const uint8_t *bound; /* host bytes: end (ascending) or start (descending), :340-347 */
  uint64_t bound_len;
} okv_merge_opts;

/* Output rows in iteration order: which input and row, and optionally an
 * index-only SoA whose offsets are relative to key_base / val_base (callers pass
 * the lowest input arena address), so the result feeds okv_encode_rows directly.
 * Any array pointer may be NULL. */
typedef struct okv_merge_out {
  uint32_t *src;
  uint64_t *row;
  uint64_t *key_off;
  uint16_t *key_len;
  uint64_t *val_off;
  uint32_t *val_len;
  const uint8_t *key_base;
  const uint8_t *val_base;
  uint64_t row_cap;
  /* filled on return: */
  uint64_t n_rows;   /* rows returned (set also with OKV_E_CAPACITY) */
  uint64_t n_unique; /* distinct keys across the inputs */
  int32_t status;    /* 0, or OKV_M_EOF (no rows are written) */
  int32_t pad;
} okv_merge_out;

/* flags: OKV_F_DEVICE_PTRS (required), OKV_F_ASYNC. At most 64 inputs. */
int okv_merge_rows(okv_ctx *ctx, const okv_merge_src *srcs, uint32_t nsrc,
                   const okv_merge_opts *opts, okv_merge_out *out, uint32_t flags);

/* ======================================================================== *
 * Range reads from resident segments: the two device steps either side of
 * okv_merge_rows when Reader.GetRange is served from segments that stay on the
 * device.  okv_seek_rows positions the streams (RowIter.Seek and the first Next,
 * segment_row_iter.go:102-207), okv_gather_rows packs the rows the merge picked.
 * DESIGN.md 23.
 * ======================================================================== */

/* A resident segment as the seek reads it: the decoded rows' keys (offsets into
 * key_arena; for an index-only decode that is the segment itself) and the first row
 * of every block, the decode's row_start.  Device pointers; the rows ascend by key
 * and block_first_row has n_blocks + 1 entries, the last one n_rows. */
typedef struct okv_seek_src {
  const uint8_t *key_arena;
  const uint64_t *key_off;
  const uint16_t *key_len;
  const uint64_t *block_first_row;
  uint64_t n_rows;
  uint64_t n_blocks;
} okv_seek_src;

/*
 * For triple i = (src_of[i], key i of `keys`, direction[i]): the rows
 * [row_lo[i], row_hi[i]) that RowIter(direction).Seek(key) followed by Next() to the
 * end yields, in ascending row numbers (a descending stream is consumed from
 * row_hi - 1): the okv_merge_src range.  An empty key is UnboundStart, the key 0xff
 * UnboundEnd.  Ascending: from the first row >= key to the end (UnboundEnd: nothing).
 * Descending: the walk starts at the last row of the last block whose FirstKey <= key
 * -- of the block before it when that FirstKey equals the key and it is not block 0
 * (DescendLessOrEqual keeps walking, :113-116), which skips that row -- and yields the
 * rows <= key from there down; UnboundStart and a key below every block yield nothing.
 * srcs is a host array (at most 65535 sources); of `keys` only key_arena, key_off,
 * key_len, n_rows and key_arena_bytes are read; fewer than 2^32 triples; n_rows == 0
 * succeeds and launches nothing.  src_of[i] >= nsrc: OKV_E_ARG in host mode, an empty
 * range with OKV_F_DEVICE_PTRS.
 * flags: without OKV_F_DEVICE_PTRS the key arrays, src_of, direction, row_lo and row_hi
 * are host memory (staged; the call synchronises); with it they are device memory and,
 * with OKV_F_ASYNC, the call only enqueues.
 */
int okv_seek_rows(okv_ctx *ctx, const okv_seek_src *srcs, uint32_t nsrc, const okv_rows *keys,
                  const uint32_t *src_of, const uint8_t *direction, uint64_t *row_lo,
                  uint64_t *row_hi, uint32_t flags);

typedef struct okv_gather_out {
  uint64_t *key_pos;  /* [n] offset of the key in key_arena, 16-byte aligned */
  uint16_t *key_len;  /* [n] */
  uint64_t *val_pos;  /* [n] offset of the value in val_arena, 16-byte aligned */
  uint32_t *val_len;  /* [n] 0 <=> Go nil */
  uint8_t *key_arena; /* or NULL (sizes only); every key zero-padded to 16 bytes; a device
                         arena must be 16-byte aligned */
  uint8_t *val_arena; /* likewise */
  uint64_t key_cap;
  uint64_t val_cap;
  /* filled on return (also with OKV_E_CAPACITY, then neither arena is written): */
  uint64_t key_bytes;
  uint64_t val_bytes;
} okv_gather_out;

/*
 * Rows (src[i], row[i]), i < n -- what okv_merge_out.src / .row hold, so nothing goes
 * to the host between merge and gather -- copied into packed arenas.  Of every
 * okv_merge_src only the six array pointers are read (row_lo, row_hi and level are
 * not); srcs is a host array of device pointers, at most 65535.  The arenas of a source
 * must be 16-byte aligned; the copy reads the aligned 16-byte lines that hold a byte of
 * the key or value, nothing else.  src and row are device memory always (src[i] >= nsrc
 * gives an empty row).  flags: without OKV_F_DEVICE_PTRS the outputs are host memory
 * (staged; the call synchronises); with it they are device memory; OKV_F_ASYNC is not
 * taken (the totals come back with the call).  n == 0 succeeds and launches nothing.
 * Returns OKV_OK, OKV_E_CAPACITY (an arena was given and key_bytes > key_cap or
 * val_bytes > val_cap: the totals and the four per-row arrays are set, the arenas are
 * not written; a call with both arenas NULL is the size query and returns OKV_OK), or
 * an error.  Fewer than 2^32 rows.
 */
int okv_gather_rows(okv_ctx *ctx, const okv_merge_src *srcs, uint32_t nsrc, const uint32_t *src,
                    const uint64_t *row, uint64_t n, okv_gather_out *out, uint32_t flags);

/* ======================================================================== *
 * Batched GetRange merge: every page of a batch of range queries in one launch.
 * A page is one OKV_MERGE_GETRANGE merge of at most OKV_PAGE_MAX_ROWS rows; one
 * workgroup runs it in LDS and nothing goes to the host inside the call.
 * DESIGN.md 24.
 * ======================================================================== */
#define OKV_PAGE_MAX_ROWS 2048  /* rows of all streams of one page */
#define OKV_M_BIG 2             /* okv_pages_out.status: the page has more rows than
                                   OKV_PAGE_MAX_ROWS; nothing was merged, use okv_merge_rows */
#define OKV_M_CAPACITY 3        /* n_rows > out_cap: n_rows is set, no row is written */

typedef struct okv_page {      /* one OKV_MERGE_GETRANGE merge; 48 bytes */
  uint64_t limit;              /* > 0 */
  uint64_t out_at;             /* first slot of this page in okv_pages_out.src / .row */
  uint64_t out_cap;            /* slots it may write */
  uint32_t src_at, nsrc;       /* its streams: srcs[src_at, src_at + nsrc), priority order, nsrc <= 64 */
  uint32_t bound_at, bound_len;/* its bound in `bounds` (end ascending, start descending), <= 65535 */
  uint32_t direction;          /* OKV_DIR_* */
  uint32_t pad;
} okv_page;

typedef struct okv_pages_out {
  uint32_t *src;      /* device: srcs index (src_at + stream), iteration order, from out_at */
  uint64_t *row;      /* device */
  uint32_t *n_rows;   /* [n_pages] rows returned (as okv_merge_out.n_rows) */
  uint32_t *n_unique; /* [n_pages] */
  int32_t  *status;   /* [n_pages] 0, OKV_M_EOF, OKV_M_BIG, OKV_M_CAPACITY */
} okv_pages_out;

/*
 * Page i is okv_merge_rows in OKV_MERGE_GETRANGE mode over srcs[src_at, src_at + nsrc):
 * the same n_rows, n_unique, status and rows, and everything that call relies on (rows
 * strictly ascending within a stream, non-empty keys, an input with row_lo == row_hi
 * ignored) carries over.  The rows go to src / row from slot out_at on; src holds the
 * index into this call's srcs (src_at + stream), so okv_gather_rows over srcs takes the
 * arrays of the whole batch as they are.  Every slot of [out_at, out_at + out_cap) that
 * holds no row gets src = 0xffffffff (okv_gather_rows' empty row), its row is not
 * written: the whole slice when status is OKV_M_EOF, OKV_M_BIG or OKV_M_CAPACITY.  Slots
 * outside every slice are not touched.  The slices of two pages must not overlap (the
 * caller's duty); pages may share streams.  A page whose streams hold more than
 * OKV_PAGE_MAX_ROWS rows gets OKV_M_BIG and the call still returns OKV_OK.
 * srcs, pages and bounds are host memory always (at most 65535 sources, fewer than 2^32
 * pages; of a page's pad nothing is read); src and row are device memory always.
 * flags: without OKV_F_DEVICE_PTRS n_rows, n_unique and status are host memory and the
 * call synchronises once, at its end; with it they are device memory and, with
 * OKV_F_ASYNC, the call only enqueues.  n_pages == 0 succeeds and launches nothing.
 * OKV_E_ARG (nothing is launched): a NULL pointer where one is needed, a page with
 * nsrc > 64, src_at + nsrc > nsrc of the call, limit == 0, a direction that is no
 * OKV_DIR_*, bound_at + bound_len > bounds_len, bound_len > 65535, or a source with
 * row_hi < row_lo.
 */
int okv_merge_pages(okv_ctx *ctx, const okv_merge_src *srcs, uint32_t nsrc,
                    const okv_page *pages, uint32_t n_pages,
                    const uint8_t *bounds, uint64_t bounds_len,
                    okv_pages_out *out, uint32_t flags);

/* Per-kernel timing with HIP events recorded on the context stream around
 * each stage of okv_decode_blocks.  okv_profile(ctx, 1) enables and resets;
 * okv_profile_read synchronises the stream and returns the summed
 * milliseconds per stage, ms[4] = {pass 1 count, pass 2 scan, pass 3 gather
 * (+ big-block copy / index), zstd decompression (0 for uncompressed)}, and
 * the number of decode calls timed.  ms must hold 4 doubles (ABI 2 and later;
 * ABI 1 wrote 3). */
int okv_profile(okv_ctx *ctx, int enable);
int okv_profile_read(okv_ctx *ctx, double *ms, uint64_t *calls);

/* The pass-3 kernels the context's last okv_decode_blocks call launched (a
 * bitmask of OKV_PATH_*), for tests and benchmarks that must show which
 * shipping kernel ran.  Set before the call returns, async or not. */
#define OKV_PATH_FUSED 1u  /* okv_decode_fused_kernel: passes 1-3 in one launch */
#define OKV_PATH_SMALL 2u  /* okv_gather_small_kernel: one wave per small block */
#define OKV_PATH_TILE 4u   /* okv_tile_kernel: large blocks, source tiles */
#define OKV_PATH_SWEEP 8u  /* okv_rows_kernel + okv_value_sweep_kernel */
#define OKV_PATH_STAGED 16u /* okv_gather_staged_kernel as the pass */
#define OKV_PATH_GATHER 32u /* okv_gather_kernel (unstaged) */
#define OKV_PATH_BIG 64u    /* okv_copy_kernel / okv_index_kernel for big blocks (always
                               launched after a non-fused pass; exits when none) */
#define OKV_PATH_ZSTD 128u  /* the zstd stage ran first */
#define OKV_PATH_STREAM 1024u   /* okv_decode_stream_kernel (ablation builds only,
                                     OKV_DECODE_STREAM=1): passes 1-3 in one launch for any batch
                                     of small blocks, prefix by decoupled look-back */
#define OKV_PATH_ENC_ONEPASS 512u /* okv_encode_rows used the single-pass plan kernel: ablation
                                     builds only (OKV_ENC_ONEPASS=1); the product runs E1-E9 */
#define OKV_PATH_ZSTD_REGROW 256u /* zstd frames outgrew their first output region and were
                                     measured and decoded again (io.Copy inflates them all) */
#define OKV_PATH_GROUP 4096u /* okv_group_kernel (ablation builds only, OKV_DECODE_GROUP=1):
                                  a large batch of small blocks in one pass, 16 blocks per
                                  workgroup, the prefix by decoupled look-back; measured
                                  slower than passes 1-3 */
#define OKV_PATH_POINT 2048u /* okv_point_kernel: a host-mode call of a few small uncompressed
                                blocks (GetRow, GetRange) in one launch over pinned memory */
#define OKV_PATH_GET 8192u /* okv_get_rows: okv_get_locate_kernel, the grouping and
                             okv_get_search_kernel */
#define OKV_PATH_ZSTD_HUF 65536u /* OKV_F_ZSTD_HUFFMAN: at least one unit of the call was written
                                    with a Compressed_Literals_Block (okv_zenc_unit_huf_kernel),
                                    whichever way its tree is described */
#define OKV_PATH_ZSTD_HUF_FSE 131072u /* OKV_F_ZSTD_HUF_FSE: at least one unit of the call was
                                         written with an FSE-compressed tree description
                                         (okv_zenc_unit_fse_kernel) */
#define OKV_PATH_ZSTD_ENC 16384u /* okv_encode_rows compressed the blocks on the device
                                    (OKV_F_ZSTD_NATIVE: okv_zenc_unit_kernel and its placement) */
#define OKV_PATH_SNAP_GET 32768u /* okv_snap_get_rows: route, locate, the grouping, the search
                                    and okv_snap_resolve_kernel */
uint32_t okv_last_path(const okv_ctx *ctx);

/* Device / pinned-host memory helpers for callers without another allocator. */
void *okv_device_alloc(okv_ctx *ctx, size_t bytes);
void okv_device_free(okv_ctx *ctx, void *p);
void *okv_host_alloc(size_t bytes); /* pinned (hipHostMalloc) */
void okv_host_free(void *p);
int okv_memcpy(okv_ctx *ctx, void *dst, const void *src, size_t bytes, int kind /*0 H2D, 1 D2H, 2 D2D*/);

#ifdef __cplusplus
}
#endif
#endif /* OKV_SST_H */
