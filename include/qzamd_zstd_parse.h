/*
 * qzamd_zstd_parse.h — how a zstd session (qzamd_zstd.h, qzamd_zstd_dec.h with QZ_DIR_BOTH) finds the sequences of its
 * frames.  Without this call they come from the parse of LZ4s sessions: one candidate per position, no offset above 65535.
 * With a depth they come from a hash-chain lazy parse cut for zstd: up to `depth` candidates per position, offsets back to
 * the chunk's first byte (131071 in a chunk of 128 KB), matches weighed by what their offsets cost, the repeat offsets among
 * them.  The frame layout, qzMaxCompressedLength, the delivery rules, crc and the totals are the same under every depth,
 * and any zstd decoder reads the frames.  Independent of qzamd_zstd_seq.h: either call may come first, neither resets the
 * other, and the sequences of a depth are the same under every setting of the sequence flags.  An addition of this
 * library.  Rules, cost and ratios: INTEGRATION.md, "Parse depth".
 */
#ifndef QZAMD_ZSTD_PARSE_H
#define QZAMD_ZSTD_PARSE_H
#include "qatzip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QZ_ZSTD_PARSE_DEPTH_MAX 256u

/* 0: the parse of today.  1..256: search attempts per position of the hash-chain lazy parse.
 * Called after setup; the calls that compress afterwards use `depth`, a later call replaces it, 0 restores the default.
 * QZ_OK on a session made by qzSetupSessionZstdAMD, or by qzSetupSessionZstdDecAMD with QZ_DIR_BOTH; QZ_PARAMS for a NULL
 * session, one that is not set up or is torn down, any other kind of session (LZ4s, decode-only zstd, deflate, LZ4) and for
 * a depth above 256. */
int qzSetSessionZstdParseAMD(QzSession_T *sess, unsigned int depth);

#ifdef __cplusplus
}
#endif
#endif
