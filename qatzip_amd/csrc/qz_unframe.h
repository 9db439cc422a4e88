/* qz_unframe.h — the host rules of qz_api.cpp's decompress calls, once each: the member header, sized gzip-ext members, one
 * member as one inflate segment, frame extents, the frame plan and its result check, the folds of the crc out-parameter.  The
 * read side of qz_frame.h, and a file of its own because that one is the write side and complete as it is.  Plain C++, no HIP
 * call, no session: tests/c/qz_unframe_test.cpp runs it under a sanitizer. */
#ifndef QZ_UNFRAME_H
#define QZ_UNFRAME_H
#include <vector>
#include "../../include/qzamd_device.h" /* the segment and result records of the device calls */
#include "qz_frame.h"

static inline uint32_t rd16(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

/* ------------------------------------------------------------------ members */
/* parse one member header at p[0..n): returns payload offset or a negative QZ_* code;
 * for gzip-ext also the sizes its extra field carries (0 when absent) */
static inline int parse_header(int fmt, const unsigned char *p, uint32_t n, uint32_t *ext_src, uint32_t *ext_dst)
{
    *ext_src = *ext_dst = 0;
    if (fmt == F_RAW) return 0;
    if (fmt == F_4B) return n >= 4 ? 4 : QZ_DATA_ERROR;
    if (fmt == F_ZLIB) {
        if (n < 2 || (p[0] & 0x0f) != 8 || ((p[0] << 8 | p[1]) % 31) || (p[1] & 0x20)) return QZ_DATA_ERROR;
        return 2;
    }
    if (n < 10 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || (p[3] & 0xe0)) return QZ_DATA_ERROR;
    uint32_t pos = 10; unsigned flg = p[3];
    if (flg & 4) {
        if (pos + 2 > n) return QZ_DATA_ERROR;
        uint32_t xl = rd16(p + pos);
        if (pos + 2 + xl > n) return QZ_DATA_ERROR;
        if (xl == 12 && p[pos + 2] == 'Q' && p[pos + 3] == 'Z' && rd16(p + pos + 4) == 8) { *ext_src = rd32(p + pos + 6); *ext_dst = rd32(p + pos + 10); }
        pos += 2 + xl;
    }
    if (flg & 8) { while (pos < n && p[pos]) pos++; pos++; }
    if (flg & 16) { while (pos < n && p[pos]) pos++; pos++; }
    if (flg & 2) pos += 2;
    return pos <= n ? (int)pos : QZ_DATA_ERROR;
}

/* a sized member: gzip-ext with both sizes in its header (qzGzipHeaderGen, src/qatzip_gzip.c:86-118) - the payload's offset,
 * its compressed and its uncompressed length.  Whether payload and trailer lie within n is the caller's question. */
struct QzSized { uint32_t pay, csz, usz; };
static inline bool qz_sized_member(const unsigned char *p, uint32_t n, QzSized *m)
{
    uint32_t es = 0, ed = 0;
    const int hl = parse_header(F_GZIP_EXT, p, n, &es, &ed);
    if (hl < 0 || es == 0 || ed == 0) return false;
    m->pay = (uint32_t)hl; m->csz = ed; m->usz = es;
    return true;
}
/* larger than any hw_buff_sz: a multi-chunk member of the software path (qzCompress fills the sizes in for those too) - the
 * member loop cuts it at its flush markers */
#define QZ_SIZED_MAX (512u * 1024u)
/* hop header to header over src[0..n): the leading sized members whose output fits cap, `pay` from src; returns the end of the last */
static inline uint32_t qz_sized_walk(const unsigned char *src, uint32_t n, uint32_t cap, std::vector<QzSized> *mem)
{
    uint32_t pos = 0; uint64_t out = 0;
    while (pos < n) {
        QzSized m;
        if (!qz_sized_member(src + pos, n - pos, &m)) break;        /* not a sized member (e.g. a software-path stream) */
        if ((uint64_t)pos + m.pay + m.csz + 8 > n) break;           /* cut short: the caller comes back with more */
        if (out + m.usz > cap) break;                               /* destination full: whole members only */
        if (m.usz > QZ_SIZED_MAX) break;
        m.pay += pos;
        mem->push_back(m);
        pos = m.pay + m.csz + 8; out += m.usz;
    }
    return pos;
}
/* the request p[0..src_len) is exactly one sized member of at most max bytes that dest_len holds */
static inline bool qz_lone_sized_member(const unsigned char *p, uint32_t src_len, uint32_t dest_len, uint32_t max, QzSized *m)
{ return qz_sized_member(p, src_len, m) && (uint64_t)m->pay + m->csz + 8 == src_len && m->usz <= dest_len && m->usz <= max; }

/* one member as one inflate segment and one CRC range */
static inline void qz_member_seg(qzd_infseg *g, qzd_range *r, uint64_t in_off, uint32_t csz, uint64_t out_off, uint32_t usz)
{
    g->in_off = in_off; g->in_len = csz; g->out_off = out_off; g->out_cap = usz;
    g->flags = 0; g->pad = csz;                                     /* exact compressed length: lets phase A split it */
    r->off = out_off; r->len = usz; r->pad = 0;
}
/* ... and what came of it against the trailer behind its payload: all of the input, all of the output, CRC-32 and ISIZE */
static inline bool member_ok(const qzd_infres &res, uint32_t c32, const unsigned char *trailer, uint32_t csz, uint32_t usz)
{ return res.status == 0 && res.out_len == usz && res.in_used == csz && rd32(trailer) == c32 && rd32(trailer + 4) == usz; }

/* ------------------------------------------------------------------ frames */
/* a frame's extent at p[0..n): its total length, < 0 when malformed or cut; its content size if the header has one; how far
 * its blocks can reach at most (qzd_zd_frame_extent of qzd_zstdd_host.h is the other one) */
typedef int64_t (*QzExtentFn)(const uint8_t *p, uint64_t n, uint64_t *content, bool *has_content, uint64_t *bound);

/* walk one LZ4 frame; an LZ4 block header says nothing about what the block decodes to, so the bound is none at all */
static inline int64_t lz4_frame_extent(const uint8_t *p, uint64_t n, uint64_t *content, bool *has_content, uint64_t *bound)
{
    *bound = UINT64_MAX;
    if (n < 7 || rd32(p) != 0x184D2204u) return -1;
    unsigned flg = p[4];
    if ((flg >> 6) != 1) return -1;
    uint32_t pos = 6;
    *has_content = (flg >> 3) & 1; *content = 0;
    if (*has_content) { if (n < 14) return -1; *content = (uint64_t)rd32(p + 6) | (uint64_t)rd32(p + 10) << 32; pos += 8; }
    if (flg & 1) pos += 4;
    pos += 1;
    for (;;) {
        if (pos + 4 > n) return -1;
        uint32_t bh = rd32(p + pos); pos += 4;
        if (bh == 0) break;
        uint32_t bsz = bh & 0x7fffffffu;
        if (bsz > n - pos) return -1;
        pos += bsz + ((flg >> 4) & 1 ? 4 : 0);
    }
    if ((flg >> 2) & 1) { if (pos + 4 > n) return -1; pos += 4; }
    return pos;
}

/* The frame loop (src/qatzip_sw.c:555-571): the leading frames of src[0..n) whose content sizes fit cap one behind the other,
 * a segment each, and ti, the input they cover.  A frame without a content size gets the rest of cap, as far as its blocks can
 * reach, and ends the plan - sizes are unknown beyond it - as `alone`.  QZ_FAIL: the first frame is malformed or cut;
 * QZ_BUF_ERROR: it does not fit; a later such frame ends the plan, and the caller comes back with the rest.
 * With `walk` instead of `extent` (qzd_zd_frame_walk: the same walk, which also counts the frame's blocks) nblocks holds a
 * count per segment, for the block route of the zstd decoder. */
typedef int64_t (*QzWalkFn)(const uint8_t *p, uint64_t n, uint64_t *content, bool *has_content, uint64_t *bound, uint32_t *nblocks);
struct QzFramePlan { std::vector<qzd_lz4seg> segs; uint32_t ti; bool alone; std::vector<uint32_t> nblocks; };
static inline int qz_frame_plan_counted(QzExtentFn extent, QzWalkFn walk, const unsigned char *src, uint32_t n, uint32_t cap, QzFramePlan *pl)
{
    uint64_t to = 0;
    pl->segs.clear(); pl->ti = 0; pl->alone = false; pl->nblocks.clear();
    while (pl->ti < n && to < cap) {
        uint64_t content, bound; bool hc;
        uint32_t nb = 0;
        const int64_t ext = walk ? walk(src + pl->ti, n - pl->ti, &content, &hc, &bound, &nb) : extent(src + pl->ti, n - pl->ti, &content, &hc, &bound);
        if (ext < 0) { if (pl->segs.empty()) return QZ_FAIL; break; }
        if (!hc) content = cap - to < bound ? cap - to : bound;
        if (to + content > cap) { if (pl->segs.empty()) return QZ_BUF_ERROR; break; }
        qzd_lz4seg g; g.in_off = pl->ti; g.out_off = to; g.in_len = (uint32_t)ext; g.out_cap = (uint32_t)content;
        pl->segs.push_back(g);
        if (walk) pl->nblocks.push_back(nb);
        pl->ti += (uint32_t)ext; to += content;
        if (!hc) { pl->alone = true; break; }
    }
    return QZ_OK;
}
static inline int qz_frame_plan(QzExtentFn extent, const unsigned char *src, uint32_t n, uint32_t cap, QzFramePlan *pl)
{
    return qz_frame_plan_counted(extent, NULL, src, n, cap, pl);
}

/* Which segment of a plan may come out shorter than its out_cap.  Every other one has to fill it, or the next frame's output
 * would not lie behind it.  The two codecs differ because their kernels do: */
enum QzShortRule {
    QZ_SHORT_LAST,                  /* LZ4: the last one, with or without a content size - the LZ4 kernels do not compare a frame's
                                     * content size with what its blocks produce, so a short last frame is nobody's error */
    QZ_SHORT_LAST_UNSIZED           /* zstd: the last one only when it had no content size (`alone`): its out_cap was a guess */
};
/* the results of a plan's n segments: the bytes produced, one behind the other from 0, or -1 when a frame failed, left input
 * over, or came short where the rule does not allow it */
static inline int64_t qz_frames_produced(const qzd_lz4seg *segs, const qzd_lz4res *res, size_t n, bool alone, QzShortRule rule)
{
    uint64_t produced = 0;
    for (size_t i = 0; i < n; i++) {
        const bool may_be_short = i + 1 == n && (rule == QZ_SHORT_LAST || alone);
        if (res[i].status != 0 || res[i].in_used != segs[i].in_len) return -1;
        if (!may_be_short && res[i].out_len != segs[i].out_cap) return -1;
        produced = segs[i].out_off + res[i].out_len;
    }
    return (int64_t)produced;
}

/* ------------------------------------------------------------------ the crc out-parameter
 * c is the CRC-32 of len bytes of output.  A member of a call: only the call's first output (to == 0) may take */
static inline void qz_crc_fold_member(unsigned long *crc, uint64_t to, uint32_t c, uint64_t len)
{ *crc = (to == 0 && *crc == 0) ? c : qzd_crc32_combine((uint32_t)*crc, c, len); }
/* a call's only output - a request of a batch, the first piece of a held member: a *crc of 0 takes */
static inline void qz_crc_fold_lone(unsigned long *crc, uint32_t c, uint64_t len)
{ *crc = *crc == 0 ? c : qzd_crc32_combine((uint32_t)*crc, c, len); }
/* a later piece of a held member: always combined */
static inline void qz_crc_fold_piece(unsigned long *crc, uint32_t c, uint64_t len)
{ *crc = qzd_crc32_combine((uint32_t)*crc, c, len); }
#endif
