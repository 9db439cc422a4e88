/*
 * qzamd_zstd_dec.h — zstd decode sessions: qzDecompress reads zstd frames (RFC 8878, no dictionaries) on the device, what
 * the ZSTD_decompressStream loop of the reference's utils/qzstd.c (decompressFile) does on the CPU.  An addition of this
 * library beside qzamd_zstd.h, which stays as it is.  Scope, refusals and scratch: INTEGRATION.md, "Zstd sessions".
 */
#ifndef QZAMD_ZSTD_DEC_H
#define QZAMD_ZSTD_DEC_H
#include "qatzip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sets up `sess` as a zstd session that decodes.  params as for qzSetupSessionZstdAMD, except that direction is
 * QZ_DIR_DECOMPRESS or QZ_DIR_BOTH (QZ_DIR_COMPRESS is QZ_PARAMS here: qzSetupSessionZstdAMD is that session); NULL: the
 * current LZ4s defaults with comp_algorithm QZ_LZ4s - their direction decides as above.  QZ_PARAMS for a hw_buff_sz above
 * 128 KB and for a non-NULL qzCallback, as there.
 *
 * The compress calls of such a session are those of a qzSetupSessionZstdAMD session with the same parameters, byte for byte.
 * qzDecompress, qzDecompressExt, qzDecompressCrc and qzDecompressCrcExt take a source of zstd frames and skippable frames
 * back to back - any writer's, not only this library's - and behave as on an LZ4 session: whole frames only; when a later
 * frame is cut or does not fit dest, the complete ones before it are delivered with QZ_OK and *src_len says where to come
 * back; QZ_FAIL when the first frame is cut, malformed, corrupt or fails its content checksum, QZ_BUF_ERROR when dest does
 * not hold the first frame; a frame without Frame_Content_Size gets the rest of dest (as far as its blocks can reach) and is
 * decoded alone, so the call returns at its end.  crc is not computed (as on an LZ4 session).  qzDecompressStream,
 * qzDecompress2, the Crc64 and the metadata calls stay refused as on every LZ4s session. */
int qzSetupSessionZstdDecAMD(QzSession_T *sess, QzSessionParamsLZ4S_T *params);

#ifdef __cplusplus
}
#endif
#endif
