/*
 * qzamd_zstd.h — zstd sessions: what the reference reaches with an LZ4s session plus the post-processing callback of its
 * utils/qzstd.c (decLz4Block, then libzstd's ZSTD_compressSequences: one zstd frame per hw_buff_sz chunk), written on the
 * device.  An addition of this library; qatzip.h is the reference's, verbatim.  Format, bound and what is refused:
 * INTEGRATION.md, "Zstd sessions".
 */
#ifndef QZAMD_ZSTD_H
#define QZAMD_ZSTD_H
#include "qatzip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sets up `sess` as a zstd session.  params as for qzSetupSessionLZ4S (comp_algorithm QZ_LZ4s, direction QZ_DIR_COMPRESS,
 * lz4s_mini_match 3 or 4, NULL: the current defaults), checked as there; in addition QZ_PARAMS for a hw_buff_sz above
 * 128 KB (a chunk is one zstd block) and for a non-NULL qzCallback (there is nothing left to post-process).
 *
 * On such a session qzCompress, qzCompressExt, qzCompressCrc and qzCompressCrcExt write one zstd frame (RFC 8878) per
 * hw_buff_sz chunk of the call, back to back, and otherwise behave as on an LZ4s session with "frame" for "block": whole
 * frames only; QZ_BUF_ERROR with *src_len and *dest_len set to what was delivered when dest holds a leading part of the
 * frames, with both 0 when it holds none; crc and total_in over the consumed input, total_out over the frames; never
 * the shared small-call queue.  qzMaxCompressedLength is the sum over the call's chunks of c + 12.  Everything an LZ4s
 * session refuses (qzDecompress*, streams, qzCompress2, the Crc64 and metadata calls) is refused with the same codes. */
int qzSetupSessionZstdAMD(QzSession_T *sess, QzSessionParamsLZ4S_T *params);

#ifdef __cplusplus
}
#endif
#endif
