/* qz_frame.h — the host rules of qz_api.cpp's compress calls, once each: the deflate bound, the delivery rule, member framing,
 * the folds of the crc out-parameter.  Plain C++, no HIP call, no session: tests/c/qz_frame_test.cpp runs it under a sanitizer. */
#ifndef QZ_FRAME_H
#define QZ_FRAME_H
#include <stdint.h>
#include <string.h>
#include "../../include/qatzip.h"
#include "qzd_slot_host.h"              /* qzd_lz4_linked_bound: shared with the device layer */

enum { F_4B = 0, F_GZIP, F_GZIP_EXT, F_RAW, F_LZ4, F_LZ4S, F_ZLIB };   /* DataFormatInternal_T order, src/qatzip_internal.h:238-253 */

static inline void wr32(unsigned char *p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24); }
static inline void wr32be(unsigned char *p, uint32_t v) { p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v; }
static inline uint32_t rd32(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static inline unsigned hdr_len(int fmt) { return fmt == F_GZIP ? 10 : fmt == F_GZIP_EXT ? 24 : fmt == F_ZLIB ? 2 : fmt == F_4B ? 4 : 0; }
static inline unsigned ftr_len(int fmt) { return (fmt == F_GZIP || fmt == F_GZIP_EXT) ? 8 : fmt == F_ZLIB ? 4 : 0; }

/* the worst case of a deflate call: `in` bytes in nchunks chunks of hw as stored blocks of 32767 bytes, flush marker, slack */
static inline uint64_t qz_deflate_bound(uint64_t in, uint64_t nchunks, uint32_t hw) { return in + nchunks * (5ull * (hw / 32767 + 2) + 16) + 64; }

struct QzFit { uint32_t take; uint64_t bytes; };        /* leading items that fit; their bytes with their overheads, without the head */
struct QzDone { uint32_t used; int rc; };               /* what the call then answers: input bytes consumed, QZ_OK or QZ_BUF_ERROR */

/* behind `head` bytes, how many of the n items - lens[k] bytes and `per_item` of framing each - does cap hold?  `trailer`
 * bytes follow the last item (the one member of compress_deflate): when only they do not fit, the last item is given back */
static inline QzFit qz_fit(uint64_t head, uint64_t per_item, uint64_t trailer, const uint32_t *lens, uint32_t n, uint64_t cap)
{
    QzFit f = {0, 0};
    while (f.take < n && head + f.bytes + per_item + lens[f.take] <= cap) f.bytes += per_item + lens[f.take++];
    if (f.take == n && n && head + f.bytes + trailer > cap) f.bytes -= per_item + lens[--f.take];
    return f;
}
/* a call that delivered `take` of its nchunks chunks used all n bytes, or whole chunks of hw */
static inline QzDone qz_delivered(uint32_t take, uint32_t nchunks, uint32_t n, uint32_t hw)
{ return take == nchunks ? QzDone{n, QZ_OK} : QzDone{take * hw, QZ_BUF_ERROR}; }

/* A member's header; returns its length.  The SOFTWARE path's, one per stream (src/qatzip_sw.c:61-75,158-171): XFL / FLEVEL by
 * level, the sizes of gzip-ext's 'QZ' field and of 4B still zero.  hw: the HARDWARE path's (src/qatzip_gzip.c:98-143), XFL 0, OS 255. */
static inline unsigned qz_member_open(unsigned char *d, int fmt, int lvl, bool hw)
{
    static const unsigned char gz[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255}, qz[14] = {12, 0, 'Q', 'Z', 8, 0};
    static const unsigned char flg[4] = {0x01, 0x5e, 0x9c, 0xda};   /* zlib: FLEVEL by level + FCHECK, behind CMF deflate/32K window */
    if (fmt == F_GZIP || fmt == F_GZIP_EXT) {
        memcpy(d, gz, 10);
        d[8] = hw ? 0 : lvl == 9 ? 2 : lvl < 2 ? 4 : 0;             /* zlib's gzip XFL: 2 = best, 4 = fastest */
        if (fmt == F_GZIP_EXT) { d[3] = 4; memcpy(d + 10, qz, 14); }
        else if (!hw) d[9] = 3;
    }
    else if (fmt == F_4B) wr32(d, 0);
    else if (fmt == F_ZLIB) { d[0] = 0x78; d[1] = flg[lvl < 2 ? 0 : lvl < 6 ? 1 : lvl == 6 ? 2 : 3]; }
    return hdr_len(fmt);
}
/* ... and its end at `at`: the trailer (gzip: CRC-32, ISIZE; zlib: Adler-32 big-endian) and, when the call that opened the
 * member also closes it (hdr = its header, else NULL), the sizes into the gzip-ext / 4B header.  Returns the trailer's length. */
static inline unsigned qz_member_close(unsigned char *hdr, unsigned char *at, int fmt, uint32_t sum, uint32_t in_total, uint32_t body)
{
    if (fmt == F_GZIP || fmt == F_GZIP_EXT) { wr32(at, sum); wr32(at + 4, in_total); }
    if (fmt == F_ZLIB) wr32be(at, sum);
    if (hdr && fmt == F_GZIP_EXT) { wr32(hdr + 16, in_total); wr32(hdr + 20, body); }
    if (hdr && fmt == F_4B) wr32(hdr, body);
    return ftr_len(fmt);
}
/* the HARDWARE path's complete member for a chunk of cl bytes that deflated to the zl bytes at z; returns its length */
static inline unsigned qz_hw_member(unsigned char *o, int fmt, const unsigned char *z, uint32_t zl, uint32_t cl, uint32_t crc)
{
    const unsigned hl = qz_member_open(o, fmt, 0, true);
    memcpy(o + hl, z, zl);
    return hl + zl + qz_member_close(o, o + hl + zl, fmt, crc, cl, zl);
}

extern "C" uint32_t qzd_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2), qzd_adler32_combine(uint32_t ad1, uint32_t ad2, uint64_t len2);

/* The software path: the `take` leading chunks (hw bytes each) of a call of n bytes go into the stream's running sum `run` (gzip:
 * CRC-32, zlib: Adler-32), which is returned, and one by one into *crc (may be NULL; src/qatzip_sw.c:217-230): a raw session folds
 * the chunk's CRC in; other formats fold the running sum - 1 for 4B - as if it covered the call so far, and a *crc of 0 takes it. */
static inline uint32_t qz_fold_chunks(unsigned long *crc, int fmt, uint32_t run, const uint32_t *crcs, const uint32_t *adlers, uint32_t take, uint32_t n, uint32_t hw)
{
    for (uint32_t k = 0, done = 0; k < take; k++) {
        const uint32_t cl = n - k * hw < hw ? n - k * hw : hw;
        if (fmt == F_GZIP || fmt == F_GZIP_EXT) run = qzd_crc32_combine(run, crcs[k], cl);
        else if (fmt == F_ZLIB) run = qzd_adler32_combine(run, adlers[k], cl);
        done += cl;
        const uint32_t sum = fmt == F_4B ? 1u : run;
        if (crc && fmt == F_RAW) *crc = qzd_crc32_combine((uint32_t)*crc, crcs[k], cl);
        else if (crc) *crc = *crc == 0 ? sum : qzd_crc32_combine((uint32_t)*crc, sum, done);
    }
    return run;
}
/* the hardware path, per chunk k of the call: the CRC-32 of the data (src/qatzip.c:1711); only a call's first chunk takes */
static inline void qz_crc_fold_hw(unsigned long *crc, uint32_t k, uint32_t chunk_crc, uint32_t cl)
{ *crc = (*crc == 0 && k == 0) ? chunk_crc : qzd_crc32_combine((uint32_t)*crc, chunk_crc, cl); }
/* an LZ4s call: the CRC-32 of the `used` bytes it consumed, always combined */
static inline void qz_crc_fold_lz4s(unsigned long *crc, uint32_t data_crc, uint32_t used)
{ *crc = qzd_crc32_combine((uint32_t)*crc, data_crc, used); }
#endif
