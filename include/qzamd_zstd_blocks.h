/*
 * qzamd_zstd_blocks.h — the block route of the zstd decoder: a frame of many blocks (what zstd, ZSTD_compress and
 * ZSTD_compressStream write) has its blocks' bit streams read in parallel, a block per lane group, where
 * qzd_zstd_decompress_frames (qzamd_device.h) reads them one after the other on the frame's lanes.  The answers are those of
 * qzd_zstd_decompress_frames, status by status; the window copies and the content checksum stay one wave per frame.  An
 * addition beside qzamd_device.h, which stays as it is.  INTEGRATION.md, "Zstd sessions", decoding.
 */
#ifndef QZAMD_ZSTD_BLOCKS_H
#define QZAMD_ZSTD_BLOCKS_H
#include "qzamd_device.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -6: the frame's block count is not h_nblocks[i] (the frame is not decoded) */
#define QZD_ZSTD_EHINT (-6)

/* qzd_zstd_decompress_frames with the frames' block counts: h_nblocks[i] is the number of blocks of frame i, or 0 where it
 * is not known - such a frame is decoded as qzd_zstd_decompress_frames decodes it.  NULL: no count is known, and the call
 * is qzd_zstd_decompress_frames.  Which frames with a count take the block route is the context's route (below).  A frame
 * that takes it with a wrong count answers QZD_ZSTD_EHINT; every other answer is that of qzd_zstd_decompress_frames.  The
 * route needs 112 bytes of scratch per block beside the frame's. */
int qzd_zstd_decompress_frames_ex(qzd_ctx *ctx, const uint8_t *d_comp, uint8_t *d_out, const void *h_segs,
                                  uint32_t nsegs, void *h_res, const uint32_t *h_nblocks);

/* The block counts of resident frames: a walk over each frame's header and block headers on the device, one wave per
 * frame, and one readback.  h_nblocks[i] <- the blocks of frame i, or 0 where the walk does not reach the frame's end (a
 * skippable, cut or malformed frame) - what the host's walk of the same bytes counts, but for a frame the decoder
 * refuses by its header (a dictionary id, a content size above 32 bits): 0 here.  QZD_ERR_PARAM for a NULL argument. */
int qzd_zstd_count_blocks(qzd_ctx *ctx, const uint8_t *d_comp, const void *h_segs, uint32_t nsegs, uint32_t *h_nblocks);

/* 0 auto: frames of 2 blocks and more; 1 frame: no frame; 2 blocks: every frame whose count is given, one-block frames
 * included.  A context starts with QATZIP_AMD_ZSTDD=auto|frame|blocks.  QZD_ERR_PARAM for another value. */
int qzd_zstd_decode_route(qzd_ctx *ctx, int route);

/* The same choice for a zstd decode session (qzSetupSessionZstdDecAMD, qzamd_zstd_dec.h), whose qzDecompress calls count
 * every frame's blocks while they walk the source: the calls that decompress afterwards use `route`.  Without this call
 * the session follows QATZIP_AMD_ZSTDD.  QZ_OK; QZ_PARAMS for a NULL session, one that is not set up, any other kind of
 * session and a route outside 0 .. 2. */
int qzSetSessionZstdDecodeRouteAMD(struct QzSession_S *sess, int route);

#ifdef __cplusplus
}
#endif
#endif
