/*
 * include/psn_jpeg.h -- JPEG frame ingest on the device (part of libpsn_lk.so).
 *
 * Replaces the step before the Tracker2D path: cv::imread(path, IMREAD_COLOR)
 * of every camera's frame (psn_where/main.cpp:133-151, :144), whose BGR output
 * CPSNWhere_Tracker2D::Run converts with cvtColor(BGR2GRAY)
 * (PSNWhere_Tracker2D.cpp:256-263). Baseline sequential JPEG (SOF0/SOF1,
 * 8-bit, Huffman), 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0, with or without
 * restart intervals, decoded as libjpeg's defaults do: Huffman (jdhuff.c),
 * jpeg_idct_islow (jidctint.c), fancy triangle upsampling (jdsample.c),
 * fixed-point YCbCr->RGB (jdcolor.c), stored in OpenCV's BGR order.
 *
 * Device work per frame: the entropy data is decoded into coefficient blocks,
 * one thread per 8x8 block runs the IDCT, one thread per pixel pair upsamples
 * the chroma, converts colour and writes BGR. The entropy decode has two paths:
 *   serial segments  one thread per restart interval (files with restart
 *                    markers, and streams with fill bytes or embedded markers);
 *   parallel         a stream without restart markers -- what cameras, encoders
 *                    and PIL write by default -- is cut into fixed-size
 *                    subsequences, one thread each: every subsequence is decoded
 *                    from a cold state, exit states are handed to the successor
 *                    until none changes (Huffman streams synchronise themselves),
 *                    then a prefix sum places the blocks and a last pass writes
 *                    them. Its output is the serial path's, byte for byte.
 * Results are bit-identical to oracle/jpeg_oracle.c, and to libjpeg-turbo's
 * decoder (the one PIL links) for intact files whose samples stay in range --
 * see oracle/jpeg_oracle.c for the pinning, for truncated files and out-of-range
 * samples, and for where OpenCV 2.4.6's bundled libjpeg 8 differs (subsampled
 * chroma).
 *
 * Plain C; returns 0 (PSN_LK_OK) or a negative PSN_LK_ERR_* code.
 */
#ifndef PSN_JPEG_H
#define PSN_JPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psn_jpeg_ctx psn_jpeg_ctx;

/* Frame geometry from the headers (host only, no device work). */
int psn_jpeg_info(const uint8_t *data, size_t len, int *width, int *height, int *components);

/* A decoder with its device scratch (grown on demand) and HIP stream. */
int psn_jpeg_create(int device, psn_jpeg_ctx **out);
void psn_jpeg_destroy(psn_jpeg_ctx *ctx);
const char *psn_jpeg_last_error(psn_jpeg_ctx *ctx);
int psn_jpeg_set_stream(psn_jpeg_ctx *ctx, void *hip_stream);

/* Decode into device memory: d_bgr receives height rows of width*3 bytes,
 * `stride` bytes apart. Asynchronous on the decoder's stream; `data` is copied
 * before the call returns. A batch of one (psn_jpeg_decode_batch_device below:
 * the same staging blob, the same kernel entries), but for its error texts,
 * which name no item, and psn_jpeg_batch_stats, for which it is no batch. */
int psn_jpeg_decode_device(psn_jpeg_ctx *ctx, const uint8_t *data, size_t len, uint8_t *d_bgr, int stride);
/* The same into host memory (synchronous). */
int psn_jpeg_decode(psn_jpeg_ctx *ctx, const uint8_t *data, size_t len, uint8_t *bgr, int stride);

/* ---- entropy paths ------------------------------------------------------- */

#define PSN_JPEG_PATH_SERIAL 0   /* one thread per restart segment */
#define PSN_JPEG_PATH_PARALLEL 1 /* self-synchronising subsequences */

/* What the planner chooses for a file (host only, no device work). A stream is
 * `plain` when every 0xFF of its entropy bytes is followed by 0x00 and the last
 * byte is not 0xFF (no fill bytes, no embedded marker); the parallel path takes
 * plain streams without restart intervals. */
typedef struct psn_jpeg_plan {
    int path;          /* PSN_JPEG_PATH_* */
    int segments;      /* restart segments (1 without restart intervals) */
    int plain;
    int entropy_bytes;
    int sub_bytes;     /* subsequence size (parallel path; else 0) */
    int subsequences;  /* ceil(entropy_bytes / sub_bytes) */
    int sequences;     /* groups of 256 subsequences, one workgroup each */
} psn_jpeg_plan;
int psn_jpeg_entropy_plan(const uint8_t *data, size_t len, psn_jpeg_plan *out);

/* What the last decode of a context ran. The round counters are written by the
 * kernels; sync_rounds is the largest round count of jpeg_sync_kernel over its
 * workgroups (at most 256), chain_rounds the rounds of jpeg_chain_kernel (at
 * most `sequences`), blocks the coefficient blocks of the scan that were
 * decoded. */
typedef struct psn_jpeg_stats {
    int path;
    int segments;
    int sub_bytes;
    int subsequences;
    int sequences;
    int sync_rounds;
    int chain_rounds;
    int blocks;
} psn_jpeg_stats;
/* Waits for the decoder's stream (the only call here that synchronises to read
 * the counters). */
int psn_jpeg_last_stats(psn_jpeg_ctx *ctx, psn_jpeg_stats *out);

/* Diagnostics, like psn_lk_debug_set_variant: product contexts run the planner.
 * mode 0: planner; 1: always the serial path; 2: the parallel path wherever it
 * is legal. sub_bytes 0: the default (PSN_JPEG_DEFAULT_SUB_BYTES), otherwise a
 * multiple of 4 in [4, 1024]. */
#define PSN_JPEG_DEFAULT_SUB_BYTES 64 /* measured 64 / 128 / 256 at 1080p: DESIGN section 4 */
int psn_jpeg_debug_set_entropy(psn_jpeg_ctx *ctx, int mode, int sub_bytes);
/* The coefficients of the context's last decode as its IDCT read them:
 * [blocks][64] int16 in natural order, DC prediction applied, the layout of
 * psn_jpeg_entropy_model's coef. Waits for the decoder's stream. `count` is the
 * number of int16 values `out` holds and must be 64 times the scan's block
 * count (psn_jpeg_entropy_model's stats->blocks with coef NULL); PSN_LK_ERR_ARG
 * otherwise, or when nothing has been decoded. */
int psn_jpeg_debug_read_coefficients(psn_jpeg_ctx *ctx, int16_t *out, size_t count);

/* ---- batches ------------------------------------------------------------- */

/* The frames of one frame-set (one file per camera) decoded in one device pass:
 * one pinned staging blob and one H2D copy for all items, one memset, and one
 * fixed number of kernel launches whatever n -- every kernel has one entry,
 * whose grid carries the item index and whose workgroups past an item's own
 * extent return at once. Items may differ in size, components, subsampling and
 * entropy path; every item's output is that of psn_jpeg_decode_device alone,
 * which is this decode at n = 1. */
#define PSN_JPEG_MAX_BATCH 64
typedef struct psn_jpeg_item {
    const uint8_t *data;
    size_t len;
    uint8_t *d_bgr; /* device memory: height rows of width*3 bytes, `stride` apart */
    int stride;
} psn_jpeg_item;

/* All or nothing: n in [1, PSN_JPEG_MAX_BATCH], the pointers, every item's
 * headers and its stride are checked before anything is enqueued; the first bad
 * item's error is returned with "item <index>" in psn_jpeg_last_error, and the
 * context is left as it was. Asynchronous on the decoder's stream; the files'
 * bytes are copied before the call returns. psn_jpeg_debug_set_entropy applies
 * to every item. Afterwards psn_jpeg_last_stats and
 * psn_jpeg_debug_read_coefficients speak of the batch's last item. */
int psn_jpeg_decode_batch_device(psn_jpeg_ctx *ctx, const psn_jpeg_item *items, int n);
/* psn_jpeg_last_stats / psn_jpeg_debug_read_coefficients of item `item` of the
 * context's last batch (both wait for the decoder's stream); PSN_LK_ERR_ARG when
 * the last decode was not a batch or had no such item. */
int psn_jpeg_batch_stats(psn_jpeg_ctx *ctx, int item, psn_jpeg_stats *out);
int psn_jpeg_debug_read_batch_coefficients(psn_jpeg_ctx *ctx, int item, int16_t *out, size_t count);

/* Where a batch puts each item (host only, no device work): byte offsets into
 * the staging blob, the parallel path's scratch, the coefficients and the
 * planes. Every offset is a multiple of 16; an item's entropy bytes are followed
 * by 16 zeroed bytes of its own (bytes_size >= entropy_bytes + 16), which is
 * what the kernels may read past the data. */
typedef struct psn_jpeg_batch_item_layout {
    int path;              /* PSN_JPEG_PATH_* */
    int list_index;        /* position in the parallel / serial list */
    size_t tables, segments, bytes;                 /* staging blob */
    size_t segments_size, bytes_size;
    size_t stats, states, counts, prefix, rounds;   /* scratch (states .. rounds: parallel items; else sizes 0) */
    size_t states_size, counts_size, prefix_size, rounds_size;
    size_t coef, coef_size;                          /* int16 [blocks][64] */
    size_t planes, planes_size;
} psn_jpeg_batch_item_layout;

typedef struct psn_jpeg_batch_layout {
    int n;
    int bad_item;          /* on an error: the first bad item, -1 for the call's own arguments */
    int n_parallel, n_serial;
    int parallel[PSN_JPEG_MAX_BATCH], serial[PSN_JPEG_MAX_BATCH]; /* item indices, ascending */
    /* the blob's tail: the kernels' two argument tables ([n] each) and the two lists */
    size_t ent_args, jpeg_args, lists;
    size_t blob_size, scratch_size, coef_size, planes_size;
    /* grid maxima over the items (parallel items: sequences, components) */
    int max_sequences, max_parallel_components, max_segment_groups /* ceil(segments / 64), serial items */;
    int max_block_groups /* ceil(blocks / 256) */, max_width, max_height;
    psn_jpeg_batch_item_layout item[PSN_JPEG_MAX_BATCH];
} psn_jpeg_batch_layout;
/* The planner at its defaults (psn_jpeg_entropy_plan per item). d_bgr is only
 * checked for null. plans may be NULL. */
int psn_jpeg_batch_plan(const psn_jpeg_item *items, int n, psn_jpeg_batch_layout *out, psn_jpeg_plan *plans);

/* CPU model of the entropy decode (host only): the symbol step the kernels run
 * (csrc/psn_jpeg_entropy.h) with the kernels' rounds emulated sequentially.
 * coef receives the scan's [blocks][64] coefficients in natural order, DC
 * prediction applied -- what the device hands to its IDCT. mode and sub_bytes
 * as above; mode 1 is the plain serial decode. Plain streams without restart
 * intervals only (PSN_LK_ERR_UNSUPPORTED otherwise). With coef NULL nothing is
 * decoded and stats->blocks is the scan's block count (the size of coef). */
int psn_jpeg_entropy_model(const uint8_t *data, size_t len, int mode, int sub_bytes, int16_t *coef,
                           psn_jpeg_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* PSN_JPEG_H */
