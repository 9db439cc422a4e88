/*
 * qzamd_zstd_seq.h — how a zstd session (qzamd_zstd.h, qzamd_zstd_dec.h with QZ_DIR_BOTH) codes the sequences of its
 * frames.  Without this call each of the literal-length, offset and match-length tables of a frame is Predefined or RLE
 * and every offset is written as offset + 3.  The sequences themselves, the frame layout, qzMaxCompressedLength and the
 * delivery rules are the same under every setting: only the bytes of the sequences section change, and any zstd decoder
 * reads them.  An addition of this library.  Rules and ratios: INTEGRATION.md, "Zstd sessions".
 */
#ifndef QZAMD_ZSTD_SEQ_H
#define QZAMD_ZSTD_SEQ_H
#include "qatzip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QZ_ZSTD_SEQ_FSE_TABLES     1u   /* LL / OF / ML each Predefined, RLE or FSE_Compressed, cheapest per chunk */
#define QZ_ZSTD_SEQ_REPEAT_OFFSETS 2u   /* offsets coded against the repeat-offset history (RFC 8878, 3.1.1.5) */

/* Called after setup; the calls that compress afterwards use `flags`, a later call replaces them, 0 restores the writer
 * described above.  QZ_OK on a session made by qzSetupSessionZstdAMD, or by qzSetupSessionZstdDecAMD with QZ_DIR_BOTH;
 * QZ_PARAMS for a NULL session, one that is not set up, any other kind of session (a decode-only zstd session and an LZ4s
 * session among them) and for a bit other than the two above. */
int qzSetSessionZstdSeqAMD(QzSession_T *sess, unsigned int flags);

#ifdef __cplusplus
}
#endif
#endif
