/*
 * qzk_zstdd.h — zstd frames (RFC 8878, no dictionaries) decoded on the device: what ZSTD_decompressStream is to the
 * reference's qzstd (utils/qzstd.c:441-510).  A frame is decoded in two stages, like the inflate's phase A and phase B:
 *
 *   Stage E (qzk_zstdd_entropy_kernel), the serial bit streams.  A wave takes QZK_ZD_G frames at once, QZK_ZD_L = 64 / G
 *   lanes each; inside a frame's lanes, lane 0 is the leader (frame and block headers, the sections' headers, the Huffman
 *   weights, the FSE table descriptions), lanes 0-3 read the up to four Huffman literal streams, lane 4 reads the
 *   interleaved LL/OF/ML stream, lanes 5-7 build the LL, OF and ML decode tables and all L lanes fill the Huffman lookup.
 *   The literal lanes and the sequence lane of a frame run in one loop: they read disjoint parts of the block.  The
 *   tables live in LDS per frame and stay there across the frame's blocks (Treeless literals, Repeat_Mode).  Repeat
 *   offsets are resolved here, so what leaves the stage are the frame's regenerated literals and one record
 *   {literal run, match length, distance} per sequence - plain distances - in the frame's scratch region; a block's
 *   trailing literals, a Raw block and an RLE block are records too ({n, 0, 0}, {n, 0, 0} with the bytes copied to the
 *   literals, {1, n - 1, 1}).
 *   Stage X (qzk_zstdd_exec_kernel): one wave per frame puts the records through the copy engine of qzk_lz_batch.h, exactly
 *   as qzk_lz_resolve_kernel does for the inflate.  hist is 0: no dictionaries, nothing before the frame.
 *   qzk_zstdd_xxh_kernel: one wave per frame with a content checksum compares the low 32 bits of XXH64 (seed 0, restated
 *   from its specification) of the frame's output with the four bytes behind the last block.
 *
 * No stage loads beyond a frame's in_len or stores beyond its out_cap or its scratch region; every refusal of
 * INTEGRATION.md ("Zstd sessions", decoding) is a status below.  Control flow around cross-lane operations is wave-uniform.
 */
#ifndef QZK_ZSTDD_H
#define QZK_ZSTDD_H
#include "qzk_common.h"
#include "qzk_lz_batch.h"

#ifndef QZK_ZD_G
#define QZK_ZD_G 4                  /* frames per wave of stage E (profiles/zstd_decode_resources.txt) */
#endif
#define QZK_ZD_L (64 / QZK_ZD_G)    /* lanes per frame: >= 8 */

#define QZK_ZD_EDATA (-1)           /* malformed */
#define QZK_ZD_EOUT (-2)            /* output beyond out_cap */
#define QZK_ZD_ETRUNC (-3)          /* the input ends inside the frame */
#define QZK_ZD_ECKSUM (-4)          /* content checksum mismatch */
#define QZK_ZD_EUNSUP (-5)          /* a dictionary id; a content size above 32 bits; a window exponent above 31 */

#define QZK_ZD_MAXBLK 131072u
#define QZK_ZD_HUFLOG 11

/* the layouts of qzd_lz4seg / qzd_lz4res (include/qzamd_device.h); pad carries the frame's record count from E to X */
typedef struct { uint64_t in_off, out_off; uint32_t in_len, out_cap; } qzk_zdseg;
typedef struct { int32_t status; uint32_t in_used, out_len, pad; } qzk_zdres;
/* a frame's scratch region (qzd_zstdd_host.h): byte offsets into the scratch buffer, capacities in bytes and in records */
typedef struct { uint64_t lit_off, rec_off; uint32_t lit_cap, rec_cap; } qzk_zdplan;

QZ_CONST int16_t qzk_zd_ll_norm[36] = { 4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1 };
QZ_CONST int16_t qzk_zd_of_norm[29] = { 1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1 };
QZ_CONST int16_t qzk_zd_ml_norm[53] = { 1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                        1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1 };
QZ_CONST uint8_t qzk_zd_ll_bits[36] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16 };
QZ_CONST uint32_t qzk_zd_ll_base[36] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512,
                                         1024, 2048, 4096, 8192, 16384, 32768, 65536 };
QZ_CONST uint8_t qzk_zd_ml_bits[53] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                        1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16 };
QZ_CONST uint32_t qzk_zd_ml_base[53] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
                                         33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539 };

/* what a frame keeps in LDS: tables across its blocks, and what its leader tells its other lanes about the current block */
typedef struct {
    uint32_t ll[512], of[256], ml[512];            /* FSE decode tables: symbol | bits << 8 | baseline << 16 */
    uint32_t wt[64];                               /* the Huffman weights' FSE table */
    uint16_t huf[1 << QZK_ZD_HUFLOG];              /* symbol | code length << 8, by the next hlog bits */
    int16_t norm[4][64];                           /* normalised counts: LL, OF, ML, weights */
    uint16_t nxt[4][64];
    uint16_t sstart[256];                          /* first lookup entry of every symbol */
    uint8_t w[256];                                /* Huffman weights */
    uint32_t rank[16];
    /* the frame */
    uint32_t pos, bmax, content, produced, nlit, nrec;
    uint32_t has_content, has_cksum, have_huf, have_seq, hlog, nsym, done;
    uint32_t tkind[3], tlog[3];                    /* per sequence table: 0 none, 1 predefined, 2 from the stream; its log */
    /* the block */
    uint32_t btype, last, bend;                    /* 0 Raw, 1 RLE, 2 Compressed, 3 nothing to decode */
    uint32_t huf_new, build[3], nsymb[3];
    uint32_t lit_kind;                             /* 0 none / done by the leader, 1 Raw (copy), 2 Huffman streams */
    uint32_t lit_src, lit_n, lit_regen;
    uint32_t s_off[4], s_len[4], s_cnt[4], s_dst[4], nstreams;
    uint32_t q_off, q_len, nseq;
    int32_t err, serr[8];
} qzk_zd_frame;

typedef struct { const uint8_t *base; uint32_t ptr, used; uint64_t c; } qzk_zd_bits;

/* a stream read from its end (RFC 8878, 4.1): the highest set bit of the last byte is the end mark.  Loads stay inside
 * [base, base + size) */
QZ_DEV int qzk_zd_bits_init(qzk_zd_bits *b, const uint8_t *base, uint32_t size)
{
    b->base = base; b->ptr = 0; b->used = 64; b->c = 0;
    if (size == 0) return QZK_ZD_EDATA;
    const uint32_t last = base[size - 1];
    if (last == 0) return QZK_ZD_EDATA;                             /* no end mark */
    const uint32_t hb = 31u - (uint32_t)__builtin_clz(last);
    if (size >= 8) { b->ptr = size - 8; b->c = qzk_rb_ld64(base + b->ptr); b->used = 8 - hb; }
    else {
        uint64_t c = 0;
        for (uint32_t i = 0; i < size; i++) c |= (uint64_t)base[i] << (8 * i);
        b->c = c; b->used = 8 - hb + 8 * (8 - size);
    }
    return 0;
}
QZ_DEV void qzk_zd_bits_refill(qzk_zd_bits *b)
{
    if (b->ptr >= 8) { b->ptr -= b->used >> 3; b->used &= 7; b->c = qzk_rb_ld64(b->base + b->ptr); }
    else if (b->ptr) {
        uint32_t nb = b->used >> 3;
        if (nb > b->ptr) nb = b->ptr;
        b->ptr -= nb; b->used -= 8 * nb; b->c = qzk_rb_ld64(b->base + b->ptr);
    }
}
/* k <= 32 bits; *err is set where the stream has fewer */
QZ_DEV uint32_t qzk_zd_bits_read(qzk_zd_bits *b, uint32_t k, int *err)
{
    if (b->used + k > 64) qzk_zd_bits_refill(b);
    if (b->used + k > 64) { *err = QZK_ZD_EDATA; return 0; }        /* read past its beginning */
    if (k == 0) return 0;
    const uint32_t v = (uint32_t)((b->c << b->used) >> (64 - k));
    b->used += k;
    return v;
}
QZ_DEV uint32_t qzk_zd_bits_left(const qzk_zd_bits *b) { return 8 * b->ptr + 64 - b->used; }
QZ_DEV bool qzk_zd_bits_done(const qzk_zd_bits *b) { return b->ptr == 0 && b->used == 64; }

/* 16 bits at bit `bit` of the forward field p[0 .. len), zeros behind its end */
QZ_DEV uint32_t qzk_zd_fwd16(const uint8_t *p, uint32_t len, uint32_t bit)
{
    const uint32_t b = bit >> 3;
    uint32_t v = 0;
    if (b < len) v |= p[b];
    if (b + 1 < len) v |= (uint32_t)p[b + 1] << 8;
    if (b + 2 < len) v |= (uint32_t)p[b + 2] << 16;
    return (v >> (bit & 7)) & 0xffffu;
}

/* an FSE table description (RFC 8878, 4.1.1) -> norm[0 .. *nsym), *log; returns the bytes used or < 0 */
QZ_DEV int qzk_zd_read_ncount(const uint8_t *p, uint32_t len, uint32_t max_log, uint32_t max_sym, int16_t *norm, uint32_t *nsym, uint32_t *log_out)
{
    if (len == 0) return QZK_ZD_EDATA;
    const uint32_t log = 5 + (p[0] & 15u);
    if (log > max_log) return QZK_ZD_EDATA;
    uint32_t pos = 4, n = 0;
    int32_t remaining = (1 << log) + 1, threshold = 1 << log;
    uint32_t nbits = log + 1;
    bool prev0 = false;
    while (remaining > 1) {
        if (prev0) {
            for (;;) {
                const uint32_t r = qzk_zd_fwd16(p, len, pos) & 3u;
                pos += 2;
                for (uint32_t i = 0; i < r && n < max_sym; i++) norm[n++] = 0;
                if (r != 3 || pos > 8 * len) break;
            }
        }
        if (n >= max_sym || pos > 8 * len) return QZK_ZD_EDATA;
        const int32_t mx = 2 * threshold - 1 - remaining;
        const uint32_t v = qzk_zd_fwd16(p, len, pos);
        int32_t count;
        if ((int32_t)(v & (uint32_t)(threshold - 1)) < mx) { count = (int32_t)(v & (uint32_t)(threshold - 1)); pos += nbits - 1; }
        else {
            count = (int32_t)(v & (uint32_t)(2 * threshold - 1));
            if (count >= threshold) count -= mx;
            pos += nbits;
        }
        count -= 1;
        remaining -= count < 0 ? -count : count;
        if (remaining < 1) return QZK_ZD_EDATA;                     /* the distribution overshoots its table */
        norm[n++] = (int16_t)count;
        prev0 = count == 0;
        while (remaining < threshold) { nbits--; threshold >>= 1; }
        if (pos > 8 * len) return QZK_ZD_EDATA;                     /* cut by its field's end */
    }
    *nsym = n; *log_out = log;
    return (int)((pos + 7) >> 3);
}

/* RFC 8878, 4.1.1: the decode table of a distribution that adds up to 1 << log */
QZ_DEV int qzk_zd_fse_build(const int16_t *norm, uint32_t nsym, uint32_t log, uint32_t *table, uint16_t *nxt)
{
    const uint32_t size = 1u << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint32_t high = size - 1, total = 0;
    for (uint32_t s = 0; s < nsym; s++) { const int32_t c = norm[s]; total += (uint32_t)(c < 0 ? -c : c); }
    if (total != size) return QZK_ZD_EDATA;                         /* (before a cell is written: the cells are counted by it) */
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t c = norm[s];
        if (c == -1) { table[high--] = s; nxt[s] = 1; } else nxt[s] = (uint16_t)c;
    }
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t c = norm[s];
        for (int32_t i = 0; i < c; i++) {
            table[pos] = s;
            do pos = (pos + step) & mask; while (pos > high);
        }
    }
    if (pos != 0) return QZK_ZD_EDATA;                              /* does not fill its table */
    for (uint32_t u = 0; u < size; u++) {
        const uint32_t s = table[u], x = nxt[s];
        nxt[s] = (uint16_t)(x + 1);
        const uint32_t nb = log - (31u - (uint32_t)__builtin_clz(x));
        table[u] = s | nb << 8 | ((x << nb) - size) << 16;
    }
    return 0;
}

/* FSE-compressed Huffman weights (4.2.1.2): two states taking turns until the stream is used up.  Returns the number of
 * weights (<= 255) or < 0 */
QZ_DEV int qzk_zd_weights_fse(qzk_zd_frame *F, const uint8_t *p, uint32_t len)
{
    uint32_t nsym = 0, log = 0;
    const int used = qzk_zd_read_ncount(p, len, 6, 13, F->norm[3], &nsym, &log);
    if (used < 0) return used;
    if (qzk_zd_fse_build(F->norm[3], nsym, log, F->wt, F->nxt[3])) return QZK_ZD_EDATA;
    qzk_zd_bits b;
    int err = qzk_zd_bits_init(&b, p + used, len - (uint32_t)used);
    if (err) return err;
    uint32_t st0 = qzk_zd_bits_read(&b, log, &err), st1 = qzk_zd_bits_read(&b, log, &err);
    if (err) return err;
    uint32_t n = 0;
    for (;;) {
        const uint32_t e = F->wt[st0], nb = (e >> 8) & 0xff;
        if (n >= 255) return QZK_ZD_EDATA;
        F->w[n++] = (uint8_t)e;
        if (nb > qzk_zd_bits_left(&b)) {
            if (n >= 255) return QZK_ZD_EDATA;
            F->w[n++] = (uint8_t)F->wt[st1];
            break;
        }
        st0 = (e >> 16) + qzk_zd_bits_read(&b, nb, &err);
        if (err) return err;
        const uint32_t t = st0; st0 = st1; st1 = t;                 /* the states take turns */
    }
    if (!qzk_zd_bits_done(&b)) return QZK_ZD_EDATA;
    return (int)n;
}

/* the weights F->w[0 .. nw) -> the last weight, the code's height, every symbol's first lookup entry; the lookup itself is
 * filled by all the frame's lanes (qzk_zd_huf_fill) */
QZ_DEV int qzk_zd_huf_plan(qzk_zd_frame *F, uint32_t nw)
{
    uint32_t total = 0;
    for (uint32_t w = 0; w < 16; w++) F->rank[w] = 0;
    for (uint32_t s = 0; s < nw; s++) {
        const uint32_t w = F->w[s];
        if (w > QZK_ZD_HUFLOG) return QZK_ZD_EDATA;
        if (w) { total += 1u << (w - 1); F->rank[w]++; }
    }
    if (total == 0) return QZK_ZD_EDATA;
    const uint32_t maxbits = 32u - (uint32_t)__builtin_clz(total), rest = (1u << maxbits) - total;
    if (rest & (rest - 1)) return QZK_ZD_EDATA;                     /* the weights do not add up to a power of two */
    if (maxbits > QZK_ZD_HUFLOG) return QZK_ZD_EDATA;
    const uint32_t lw = 32u - (uint32_t)__builtin_clz(rest);
    F->w[nw] = (uint8_t)lw; F->rank[lw]++;
    if (F->rank[1] < 2) return QZK_ZD_EDATA;                        /* no two symbols of weight 1: libzstd's HUF_readStats refuses it */
    uint32_t at = 0;
    for (uint32_t w = 1; w <= maxbits; w++) { const uint32_t c = F->rank[w]; F->rank[w] = at; at += c << (w - 1); }
    for (uint32_t s = 0; s <= nw; s++) {
        const uint32_t w = F->w[s];
        if (w) { F->sstart[s] = (uint16_t)F->rank[w]; F->rank[w] += 1u << (w - 1); }
    }
    F->hlog = maxbits; F->nsym = nw + 1; F->have_huf = 1; F->huf_new = 1;
    return 0;
}
QZ_DEV void qzk_zd_huf_fill(qzk_zd_frame *F, uint32_t r)
{
    for (uint32_t s = r; s < F->nsym; s += QZK_ZD_L) {
        const uint32_t w = F->w[s];
        if (!w) continue;
        const uint32_t n = 1u << (w - 1), e = s | (F->hlog + 1 - w) << 8, at = F->sstart[s];
        for (uint32_t i = 0; i < n; i++) F->huf[at + i] = (uint16_t)e;
    }
}

/* the leader, once per frame: the frame header.  Returns 0, or a status with the frame done */
QZ_DEV int qzk_zd_frame_header(qzk_zd_frame *F, const uint8_t *in, uint32_t in_len, uint32_t out_cap, uint32_t *skippable)
{
    *skippable = 0;
    if (in_len < 4) return QZK_ZD_ETRUNC;
    const uint32_t magic = in[0] | (uint32_t)in[1] << 8 | (uint32_t)in[2] << 16 | (uint32_t)in[3] << 24;
    if ((magic & 0xfffffff0u) == 0x184D2A50u) {
        if (in_len < 8) return QZK_ZD_ETRUNC;
        const uint32_t sz = in[4] | (uint32_t)in[5] << 8 | (uint32_t)in[6] << 16 | (uint32_t)in[7] << 24;
        if (sz > in_len - 8) return QZK_ZD_ETRUNC;
        F->pos = 8 + sz; *skippable = 1;
        return 0;
    }
    if (magic != 0xFD2FB528u) return QZK_ZD_EDATA;
    if (in_len < 5) return QZK_ZD_ETRUNC;
    const uint32_t fhd = in[4];
    if (fhd & 0x08) return QZK_ZD_EDATA;
    if (fhd & 0x03) return QZK_ZD_EUNSUP;
    const uint32_t single = (fhd >> 5) & 1, flag = fhd >> 6;
    const uint32_t fb = flag == 0 ? single : flag == 1 ? 2u : flag == 2 ? 4u : 8u;
    const uint32_t hs = 5 + (single ? 0u : 1u) + fb;
    if (in_len < hs) return QZK_ZD_ETRUNC;
    uint32_t p = 5;
    uint64_t window = 0;
    if (!single) {
        const uint32_t wlog = 10 + (in[p] >> 3);
        if (wlog > 31) return QZK_ZD_EUNSUP;                        /* libzstd's ZSTD_WINDOWLOG_MAX: it refuses such a frame */
        window = (1ull << wlog) + ((1ull << wlog) >> 3) * (in[p] & 7u);
        p++;
    }
    uint64_t content = 0;
    for (uint32_t i = 0; i < fb; i++) content |= (uint64_t)in[p + i] << (8 * i);
    if (fb == 2) content += 256;
    if (content > 0xffffffffull) return QZK_ZD_EUNSUP;
    if (single) window = content;
    F->has_content = fb != 0; F->content = (uint32_t)content; F->has_cksum = (fhd >> 2) & 1;
    F->bmax = window < QZK_ZD_MAXBLK ? (uint32_t)window : QZK_ZD_MAXBLK;
    F->pos = hs;
    if (fb && content > out_cap) return QZK_ZD_EOUT;
    return 0;
}

/* one record into the frame's scratch */
QZ_DEV int qzk_zd_record(uint32_t *rec, uint32_t rec_cap, uint32_t *nrec, uint32_t ll, uint32_t ml, uint32_t dist)
{
    if (*nrec >= rec_cap) return QZK_ZD_EDATA;
    uint32_t *r = rec + 3 * (size_t)*nrec;
    r[0] = ll; r[1] = ml; r[2] = dist;
    (*nrec)++;
    return 0;
}

/* the leader, once per block: the block header, the literals section's header and tree, the sequences section's header and
 * table descriptions.  What the other lanes need is left in F.  Returns 0 or a status */
QZ_DEV int qzk_zd_block(qzk_zd_frame *F, const uint8_t *in, uint32_t in_len, uint32_t out_cap, uint8_t *lit, uint32_t lit_cap,
                        uint32_t *rec, uint32_t rec_cap)
{
    uint32_t pos = F->pos;
    F->btype = 3; F->huf_new = 0; F->build[0] = F->build[1] = F->build[2] = 0; F->lit_kind = 0; F->nstreams = 0; F->nseq = 0;
    F->lit_regen = 0; F->q_len = 0;
    if (in_len - pos < 3) return QZK_ZD_ETRUNC;
    const uint32_t bh = in[pos] | (uint32_t)in[pos + 1] << 8 | (uint32_t)in[pos + 2] << 16;
    pos += 3;
    const uint32_t type = (bh >> 1) & 3, bsz = bh >> 3;
    F->last = bh & 1;
    if (type == 3) return QZK_ZD_EDATA;
    if (bsz > F->bmax) return QZK_ZD_EDATA;
    if (type != 2) {
        const uint32_t need = type == 0 ? bsz : 1u;
        if (in_len - pos < need) return QZK_ZD_ETRUNC;
        if ((uint64_t)F->produced + bsz > out_cap) return QZK_ZD_EOUT;
        if (F->has_content && F->produced + bsz > F->content) return QZK_ZD_EDATA;
        F->bend = pos + need;
        if (bsz == 0) return 0;
        if (type == 0) {
            if (bsz > lit_cap - F->nlit) return QZK_ZD_EDATA;
            int e = qzk_zd_record(rec, rec_cap, &F->nrec, bsz, 0, 0);
            if (e) return e;
            F->btype = 0; F->lit_kind = 1; F->lit_src = pos; F->lit_n = bsz; F->lit_regen = bsz;
        } else {
            if (1 > lit_cap - F->nlit) return QZK_ZD_EDATA;
            lit[F->nlit] = in[pos];
            int e = qzk_zd_record(rec, rec_cap, &F->nrec, 1, bsz - 1, 1);
            if (e) return e;
            F->btype = 1; F->lit_regen = 1;
        }
        F->produced += bsz;
        return 0;
    }
    if (in_len - pos < bsz) return QZK_ZD_ETRUNC;
    const uint8_t *b = in + pos;
    F->bend = pos + bsz;
    /* ---- literals section ---- */
    if (bsz < 1) return QZK_ZD_EDATA;
    const uint32_t t = b[0] & 3, fmt = (b[0] >> 2) & 3;
    uint32_t lend;                                                  /* where the literals section ends inside the block */
    uint32_t n;
    if (t < 2) {
        const uint32_t hs = !(fmt & 1) ? 1u : fmt == 1 ? 2u : 3u;
        if (bsz < hs) return QZK_ZD_EDATA;
        uint32_t v = b[0];
        if (hs > 1) v |= (uint32_t)b[1] << 8;
        if (hs > 2) v |= (uint32_t)b[2] << 16;
        n = v >> (hs == 1 ? 3 : 4);
        if (n > QZK_ZD_MAXBLK || n > lit_cap - F->nlit) return QZK_ZD_EDATA;
        if (t == 0) {
            if (bsz - hs < n) return QZK_ZD_EDATA;
            F->lit_kind = 1; F->lit_src = pos + hs; F->lit_n = n;
            lend = hs + n;
        } else {
            if (bsz - hs < 1) return QZK_ZD_EDATA;
            F->lit_kind = 3; F->lit_src = pos + hs; F->lit_n = n;   /* n copies of one byte, by all the frame's lanes */
            lend = hs + 1;
        }
    } else {
        const uint32_t hs = fmt < 2 ? 3u : fmt == 2 ? 4u : 5u, bits = fmt < 2 ? 10u : fmt == 2 ? 14u : 18u, streams = fmt == 0 ? 1u : 4u;
        if (bsz < hs) return QZK_ZD_EDATA;
        uint64_t v = 0;
        for (uint32_t i = 0; i < hs; i++) v |= (uint64_t)b[i] << (8 * i);
        v >>= 4;
        n = (uint32_t)(v & ((1u << bits) - 1));
        const uint32_t csz = (uint32_t)(v >> bits);
        if (n > QZK_ZD_MAXBLK || n > lit_cap - F->nlit) return QZK_ZD_EDATA;
        if (bsz - hs < csz) return QZK_ZD_EDATA;
        const uint8_t *body = b + hs;
        uint32_t dsz = 0;
        if (t == 3) { if (!F->have_huf) return QZK_ZD_EDATA; }
        else {
            if (csz < 1) return QZK_ZD_EDATA;
            const uint32_t hb = body[0];
            int nw;
            if (hb >= 128) {
                nw = (int)hb - 127;
                dsz = 1 + ((uint32_t)nw + 1) / 2;
                if (csz < dsz) return QZK_ZD_EDATA;
                for (int i = 0; i < nw; i++) { const uint32_t x = body[1 + i / 2]; F->w[i] = (uint8_t)(i & 1 ? x & 15 : x >> 4); }
            } else {
                if (hb == 0 || csz < 1 + hb) return QZK_ZD_EDATA;
                nw = qzk_zd_weights_fse(F, body + 1, hb);
                if (nw < 0) return nw;
                dsz = 1 + hb;
            }
            const int e = qzk_zd_huf_plan(F, (uint32_t)nw);
            if (e) return e;
        }
        const uint32_t roff = pos + hs + dsz, rlen = csz - dsz;
        F->lit_kind = 2; F->nstreams = streams;
        if (streams == 1) { F->s_off[0] = roff; F->s_len[0] = rlen; F->s_cnt[0] = n; F->s_dst[0] = F->nlit; }
        else {
            if (rlen < 6) return QZK_ZD_EDATA;
            const uint8_t *j = in + roff;
            const uint32_t s1 = j[0] | (uint32_t)j[1] << 8, s2 = j[2] | (uint32_t)j[3] << 8, s3 = j[4] | (uint32_t)j[5] << 8;
            const uint32_t rem = rlen - 6, seg = (n + 3) / 4;
            if (s1 + s2 + s3 >= rem) return QZK_ZD_EDATA;           /* the jump table runs past the section */
            if (n < 3 * seg) return QZK_ZD_EDATA;
            F->s_off[0] = roff + 6; F->s_len[0] = s1; F->s_off[1] = F->s_off[0] + s1; F->s_len[1] = s2;
            F->s_off[2] = F->s_off[1] + s2; F->s_len[2] = s3; F->s_off[3] = F->s_off[2] + s3; F->s_len[3] = rem - s1 - s2 - s3;
            for (uint32_t i = 0; i < 4; i++) { F->s_cnt[i] = i < 3 ? seg : n - 3 * seg; F->s_dst[i] = F->nlit + i * seg; }
        }
        lend = hs + csz;
    }
    F->lit_regen = n;
    /* ---- sequences section ---- */
    const uint8_t *q = b + lend;
    const uint32_t qlen = bsz - lend;
    if (qlen < 1) return QZK_ZD_EDATA;
    uint32_t nseq, qp;
    if (q[0] < 128) { nseq = q[0]; qp = 1; }
    else if (q[0] < 255) { if (qlen < 2) return QZK_ZD_EDATA; nseq = ((uint32_t)(q[0] - 128) << 8) + q[1]; qp = 2; }
    else { if (qlen < 3) return QZK_ZD_EDATA; nseq = q[1] + ((uint32_t)q[2] << 8) + 0x7f00; qp = 3; }
    F->btype = 2; F->nseq = nseq;
    if (nseq == 0) return qlen == 1 ? 0 : QZK_ZD_EDATA;
    if (qp >= qlen) return QZK_ZD_EDATA;
    const uint32_t modes = q[qp++];
    if (modes & 3) return QZK_ZD_EDATA;
    for (uint32_t k = 0; k < 3; k++) {
        const uint32_t mode = (modes >> (6 - 2 * k)) & 3;
        const uint32_t maxsym = k == 0 ? 35u : k == 1 ? 31u : 52u, maxlog = k == 1 ? 8u : 9u;
        if (mode == 3) { if (!F->have_seq) return QZK_ZD_EDATA; continue; }
        if (mode == 0) {
            if (F->tkind[k] == 1) continue;
            const int16_t *src = k == 0 ? qzk_zd_ll_norm : k == 1 ? qzk_zd_of_norm : qzk_zd_ml_norm;
            const uint32_t ns = k == 0 ? 36u : k == 1 ? 29u : 53u;
            for (uint32_t i = 0; i < ns; i++) F->norm[k][i] = src[i];
            F->nsymb[k] = ns; F->tlog[k] = k == 1 ? 5u : 6u; F->build[k] = 1; F->tkind[k] = 1;
        } else if (mode == 1) {
            if (qp >= qlen) return QZK_ZD_EDATA;
            const uint32_t sym = q[qp++];
            if (sym > maxsym) return QZK_ZD_EDATA;
            (k == 0 ? F->ll : k == 1 ? F->of : F->ml)[0] = sym;
            F->tlog[k] = 0; F->tkind[k] = 2;
        } else {
            uint32_t ns = 0, lg = 0;
            const int used = qzk_zd_read_ncount(q + qp, qlen - qp, maxlog, maxsym + 1, F->norm[k], &ns, &lg);
            if (used < 0) return used;
            qp += (uint32_t)used;
            F->nsymb[k] = ns; F->tlog[k] = lg; F->build[k] = 1; F->tkind[k] = 2;
        }
    }
    F->have_seq = 1;
    if (qp >= qlen) return QZK_ZD_EDATA;
    F->q_off = pos + lend + qp; F->q_len = qlen - qp;
    return 0;
}

/* Stage E.  grid: ceil(nsegs / QZK_ZD_G) single-wave workgroups */
QZ_KERNEL_MAX(64) qzk_zstdd_entropy_kernel(const uint8_t *comp, const qzk_zdseg *segs, const qzk_zdplan *plan, qzk_zdres *res,
                                           uint32_t nsegs, uint8_t *scratch)
{
    QZ_LDS qzk_zd_frame frames[QZK_ZD_G];
    const uint32_t lane = (uint32_t)qz_lane(), g = lane / QZK_ZD_L, r = lane % QZK_ZD_L;
    const uint32_t fidx = blockIdx.x * QZK_ZD_G + g;
    const bool valid = fidx < nsegs;
    qzk_zd_frame *const F = &frames[g];
    qzk_zdseg sg; sg.in_off = 0; sg.out_off = 0; sg.in_len = 0; sg.out_cap = 0;
    qzk_zdplan pl; pl.lit_off = 0; pl.rec_off = 0; pl.lit_cap = 0; pl.rec_cap = 0;
    if (valid) { sg = segs[fidx]; pl = plan[fidx]; }
    const uint8_t *const in = comp + sg.in_off;
    uint8_t *const lit = scratch + pl.lit_off;
    uint32_t *const rec = (uint32_t *)(scratch + pl.rec_off);
    if (r == 0) {
        F->pos = 0; F->bmax = 0; F->content = 0; F->produced = 0; F->nlit = 0; F->nrec = 0; F->has_content = 0; F->has_cksum = 0;
        F->have_huf = 0; F->have_seq = 0; F->hlog = 0; F->nsym = 0; F->done = 1; F->err = 0;
        F->tkind[0] = F->tkind[1] = F->tkind[2] = 0;
        if (valid) {
            uint32_t skip = 0;
            F->err = qzk_zd_frame_header(F, in, sg.in_len, sg.out_cap, &skip);
            F->done = F->err != 0 || skip;
        }
    }
    uint32_t rep0 = 1, rep1 = 4, rep2 = 8;                          /* the sequence lane's, across the frame's blocks */
    qz_wave_sync();
    while (qz_ballot(valid && !F->done) != 0) {
        const bool active = valid && !F->done;
        qz_wave_sync();                                             /* everyone has read `done` before the leader may change it */
        /* ---- 1: the leader reads the block's headers ---- */
        if (active && r == 0) {
            for (uint32_t i = 0; i < 8; i++) F->serr[i] = 0;
            F->err = qzk_zd_block(F, in, sg.in_len, sg.out_cap, lit, pl.lit_cap, rec, pl.rec_cap);
        }
        qz_wave_sync();
        const bool work = active && F->err == 0;
        /* ---- 2: the tables ---- */
        if (work && F->btype == 2) {
            if (r >= 5 && r <= 7 && F->build[r - 5]) {
                const uint32_t k = r - 5;
                F->serr[r] = qzk_zd_fse_build(F->norm[k], F->nsymb[k], F->tlog[k], k == 0 ? F->ll : k == 1 ? F->of : F->ml, F->nxt[k]);
            }
            if (F->huf_new) qzk_zd_huf_fill(F, r);
        }
        qz_wave_sync();
        /* ---- 3: the streams, one lane each; Raw and RLE bytes by all the frame's lanes ---- */
        {
            const bool tables_ok = work && F->serr[5] == 0 && F->serr[6] == 0 && F->serr[7] == 0;
            if (tables_ok && (F->lit_kind == 1 || F->lit_kind == 3)) {
                const uint32_t n = F->lit_n;
                uint8_t *d = lit + F->nlit;
                const uint8_t *s = in + F->lit_src;
                if (F->lit_kind == 1) {
                    for (uint32_t i = 8 * r; i + 8 <= n; i += 8 * QZK_ZD_L) qzk_rb_st64(d + i, qzk_rb_ld64(s + i));
                    if (r < (n & 7)) d[(n & ~7u) + r] = s[(n & ~7u) + r];
                } else {
                    const uint8_t v = s[0];
                    for (uint32_t i = r; i < n; i += QZK_ZD_L) d[i] = v;
                }
            }
            /* a Huffman lane */
            qzk_zd_bits hb; hb.base = in; hb.ptr = 0; hb.used = 64; hb.c = 0;
            uint32_t hleft = 0; uint8_t *hd = lit; int herr = 0;
            const uint32_t hlog = F->hlog;
            if (tables_ok && F->lit_kind == 2 && r < F->nstreams) {
                herr = qzk_zd_bits_init(&hb, in + F->s_off[r], F->s_len[r]);
                hleft = herr ? 0 : F->s_cnt[r]; hd = lit + F->s_dst[r];
            }
            /* the sequence lane */
            qzk_zd_bits qb; qb.base = in; qb.ptr = 0; qb.used = 64; qb.c = 0;
            uint32_t qleft = 0, sl = 0, so = 0, sm = 0, lit_used = 0, produced = F->produced, nrec = F->nrec, bprod = 0;
            int qerr = 0;
            const bool seqlane = tables_ok && F->btype == 2 && r == 4;
            if (seqlane && F->nseq) {
                qerr = qzk_zd_bits_init(&qb, in + F->q_off, F->q_len);
                if (!qerr) {
                    sl = qzk_zd_bits_read(&qb, F->tlog[0], &qerr);
                    so = qzk_zd_bits_read(&qb, F->tlog[1], &qerr);
                    sm = qzk_zd_bits_read(&qb, F->tlog[2], &qerr);
                }
                qleft = qerr ? 0 : F->nseq;
            }
            const uint32_t lit_regen = F->lit_regen;
            while (qz_ballot(hleft != 0 || qleft != 0) != 0) {
                if (hleft) {
                    for (uint32_t k = 0; k < 4 && hleft; k++) {
                        if (hb.used + hlog > 64) qzk_zd_bits_refill(&hb);
                        const uint32_t v = hb.used < 64 ? (uint32_t)((hb.c << hb.used) >> (64 - hlog)) : 0;
                        const uint32_t e = F->huf[v], nb = e >> 8;
                        if (hb.used + nb > 64) { herr = QZK_ZD_EDATA; hleft = 0; break; }      /* the stream ends inside a code */
                        hb.used += nb;
                        *hd++ = (uint8_t)e;
                        hleft--;
                    }
                }
                if (qleft) {
                    const uint32_t el = F->ll[sl], eo = F->of[so], em = F->ml[sm];
                    const uint32_t lc = el & 0xff, oc = eo & 0xff, mc = em & 0xff;
                    if (lc > 35 || oc > 31 || mc > 52) { qerr = QZK_ZD_EDATA; qleft = 0; }
                    else {
                        const uint32_t ov = (1u << oc) + qzk_zd_bits_read(&qb, oc, &qerr);
                        const uint32_t ml = qzk_zd_ml_base[mc] + qzk_zd_bits_read(&qb, qzk_zd_ml_bits[mc], &qerr);
                        const uint32_t ll = qzk_zd_ll_base[lc] + qzk_zd_bits_read(&qb, qzk_zd_ll_bits[lc], &qerr);
                        uint32_t dist;
                        if (ov > 3) { dist = ov - 3; rep2 = rep1; rep1 = rep0; rep0 = dist; }
                        else {
                            const uint32_t idx = ov - 1 + (ll == 0 ? 1u : 0u);
                            if (idx == 0) dist = rep0;
                            else {
                                dist = idx == 1 ? rep1 : idx == 2 ? rep2 : rep0 - 1;
                                if (idx != 1) rep2 = rep1;
                                rep1 = rep0; rep0 = dist;
                            }
                        }
                        lit_used += ll;
                        if (!qerr) {
                            if (dist == 0 || lit_used > lit_regen) qerr = QZK_ZD_EDATA;
                            else if ((uint64_t)produced + ll + ml > sg.out_cap) qerr = QZK_ZD_EOUT;
                            else if (dist > produced + ll) qerr = QZK_ZD_EDATA;
                            else qerr = qzk_zd_record(rec, pl.rec_cap, &nrec, ll, ml, dist);
                        }
                        produced += ll + ml; bprod += ll + ml;
                        qleft--;
                        if (qerr) qleft = 0;
                        else if (qleft) {
                            sl = (el >> 16) + qzk_zd_bits_read(&qb, (el >> 8) & 0xff, &qerr);
                            sm = (em >> 16) + qzk_zd_bits_read(&qb, (em >> 8) & 0xff, &qerr);
                            so = (eo >> 16) + qzk_zd_bits_read(&qb, (eo >> 8) & 0xff, &qerr);
                            if (qerr) qleft = 0;
                        }
                    }
                }
            }
            if (tables_ok && F->lit_kind == 2 && r < F->nstreams) {
                if (!herr && !qzk_zd_bits_done(&hb)) herr = QZK_ZD_EDATA;                       /* bits left over */
                F->serr[r] = herr;
            }
            if (seqlane) {
                if (!qerr && F->nseq && !qzk_zd_bits_done(&qb)) qerr = QZK_ZD_EDATA;
                const uint32_t rest = lit_regen - lit_used;
                if (!qerr && rest) {
                    if ((uint64_t)produced + rest > sg.out_cap) qerr = QZK_ZD_EOUT;
                    else qerr = qzk_zd_record(rec, pl.rec_cap, &nrec, rest, 0, 0);
                    produced += rest; bprod += rest;
                }
                if (!qerr && bprod > F->bmax) qerr = QZK_ZD_EDATA;
                if (!qerr && F->has_content && produced > F->content) qerr = QZK_ZD_EDATA;
                F->serr[4] = qerr; F->produced = produced; F->nrec = nrec;
            }
        }
        qz_wave_sync();
        /* ---- 4: the leader closes the block, and the frame behind its last one ---- */
        if (active && r == 0) {
            int e = F->err;
            for (uint32_t i = 0; i < 8 && !e; i++) e = F->serr[i];
            if (!e) {
                F->nlit += F->lit_regen; F->pos = F->bend;
                if (F->last) {
                    if (F->has_content && F->produced != F->content) e = QZK_ZD_EDATA;
                    else if (F->has_cksum) { if (sg.in_len - F->pos < 4) e = QZK_ZD_ETRUNC; else F->pos += 4; }
                    F->done = 1;
                }
            }
            if (e) { F->err = e; F->done = 1; }
        }
        qz_wave_sync();
    }
    if (valid && r == 0) {
        qzk_zdres o; o.status = F->err; o.in_used = F->err ? 0 : F->pos; o.out_len = F->err ? 0 : F->produced; o.pad = F->err ? 0 : F->nrec;
        res[fidx] = o;
    }
}

/* Stage X: one wave per frame; the loop of qzk_lz_resolve_kernel (qzk_inflate_lane.h) over 12-byte records */
QZ_KERNEL_OCC(64, 8) qzk_zstdd_exec_kernel(uint8_t *out, const qzk_zdseg *segs, const qzk_zdplan *plan, qzk_zdres *res, uint32_t nsegs,
                                           const uint8_t *scratch)
{
    QZ_LDS __attribute__((aligned(16))) uint8_t obuf[QZK_RB_OB];
    QZ_LDS __attribute__((aligned(16))) uint8_t lbuf[QZK_RB_LT];
    const int lane = qz_lane();
    const uint32_t f = blockIdx.x;
    if (f >= nsegs) return;
    const qzk_zdres rs = res[f];
    if (rs.status != 0 || rs.pad == 0) return;
    const qzk_zdseg sg = segs[f];
    const qzk_zdplan pl = plan[f];
    const uint8_t *lp = scratch + pl.lit_off;
    const uint32_t *rec = (const uint32_t *)(scratch + pl.rec_off);
    const uint32_t ns = rs.pad;
    qzk_rb S;
    qzk_rb_init(&S, obuf, lbuf, out + sg.out_off, 0, sg.out_cap);
    int err = 0;
    uint32_t lbase = 0, b0 = 0;
    uint32_t c0 = 0, c1 = 0, c2 = 0;
    if ((uint32_t)lane < ns) { c0 = rec[3 * lane]; c1 = rec[3 * lane + 1]; c2 = rec[3 * lane + 2]; }
    while (b0 < ns) {
        uint32_t litrun = c0, mlen = c1, dist = c2;
        uint32_t s_tot = qz_wave_incl_scan(litrun + mlen), s_lit = qz_wave_incl_scan(litrun);
        uint32_t n = qzk_rb_fit(s_tot, s_lit);
        if (n > ns - b0) n = ns - b0;
        if (n == 0) {
            /* the first record alone is more than a batch holds: straight to the output */
            const uint32_t L = qz_readlane(litrun, 0), M = qz_readlane(mlen, 0), D = qz_readlane(dist, 0);
            if ((uint64_t)S.obase + L + M > sg.out_cap) { err = -2; break; }
            if (M != 0 && (D == 0 || (uint64_t)D > (uint64_t)S.obase + L)) { err = -4; break; }
            qzk_rb_flush(&S, lane);
            qzk_rb_direct(&S, lp + lbase, L, lane);
            qz_wave_sync();
            qzk_rb_skip(&S, L);
            if (M) { qzk_rb_direct_match(&S, D, M, lane); qz_wave_sync(); qzk_rb_skip(&S, M); }
            lbase += L; b0 += 1;
            c0 = c1 = c2 = 0;
            if (b0 + (uint32_t)lane < ns) { const uint32_t *p = rec + 3 * (size_t)(b0 + (uint32_t)lane); c0 = p[0]; c1 = p[1]; c2 = p[2]; }
            continue;
        }
        uint32_t n0 = 0, n1 = 0, n2 = 0;                            /* the batch after this one: asked for now */
        if (b0 + n + (uint32_t)lane < ns) { const uint32_t *p = rec + 3 * (size_t)(b0 + n + (uint32_t)lane); n0 = p[0]; n1 = p[1]; n2 = p[2]; }
        if ((uint32_t)lane >= n) { s_tot -= litrun + mlen; s_lit -= litrun; litrun = 0; mlen = 0; }
        const uint32_t Tb = qz_readlane(s_tot, (int)n - 1), Lb = qz_readlane(s_lit, (int)n - 1);
        if (qz_ballot(mlen != 0 && dist == 0) != 0) { err = -4; break; }
        err = qzk_rb_batch(&S, lp + lbase, Lb, s_lit - litrun, litrun, mlen, dist, s_tot, Tb, lane);
        if (err) break;
        lbase += Lb; b0 += n;
        c0 = n0; c1 = n1; c2 = n2;
    }
    if (!err) qzk_rb_flush(&S, lane);
    if (!err && S.obase != rs.out_len) err = -4;
    if (err) res[f].status = err == -2 ? QZK_ZD_EOUT : QZK_ZD_EDATA;
}

/* ------------------------------------------------------------------ XXH64, from its specification */
#define QZK_XXP1 0x9E3779B185EBCA87ull
#define QZK_XXP2 0xC2B2AE3D27D4EB4Full
#define QZK_XXP3 0x165667B19E3779F9ull
#define QZK_XXP4 0x85EBCA77C2B2AE63ull
#define QZK_XXP5 0x27D4EB2F165667C5ull
QZ_DEV uint64_t qzk_xx_rotl(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
QZ_DEV uint64_t qzk_xx_round(uint64_t acc, uint64_t v) { return qzk_xx_rotl(acc + v * QZK_XXP2, 31) * QZK_XXP1; }
QZ_DEV uint64_t qzk_xx_merge(uint64_t h, uint64_t v) { return (h ^ qzk_xx_round(0, v)) * QZK_XXP1 + QZK_XXP4; }
QZ_DEV uint64_t qzk_zd_shfl64(uint64_t v, int src)
{
    const uint32_t lo = qz_shfl((uint32_t)v, src), hi = qz_shfl((uint32_t)(v >> 32), src);
    return (uint64_t)hi << 32 | lo;
}

/* one wave per frame: lanes 0-3 are the four accumulators over the 32-byte stripes, lane 0 finishes */
QZ_KERNEL_MAX(64) qzk_zstdd_xxh_kernel(const uint8_t *comp, const uint8_t *out, const qzk_zdseg *segs, qzk_zdres *res, uint32_t nsegs)
{
    const int lane = qz_lane();
    const uint32_t f = blockIdx.x;
    if (f >= nsegs) return;
    const qzk_zdres rs = res[f];
    const qzk_zdseg sg = segs[f];
    if (rs.status != 0 || rs.in_used < 9) return;
    const uint8_t *in = comp + sg.in_off;
    if (qz_ld32(in) != 0xFD2FB528u || !(in[4] & 4)) return;
    const uint8_t *p = out + sg.out_off;
    const uint32_t n = rs.out_len, stripes = n >> 5;
    uint64_t acc = lane == 0 ? QZK_XXP1 + QZK_XXP2 : lane == 1 ? QZK_XXP2 : lane == 2 ? 0 : 0 - QZK_XXP1;
    if (lane < 4) for (uint32_t i = 0; i < stripes; i++) acc = qzk_xx_round(acc, qzk_rb_ld64(p + 32 * (size_t)i + 8 * (uint32_t)lane));
    const uint64_t a1 = qzk_zd_shfl64(acc, 1), a2 = qzk_zd_shfl64(acc, 2), a3 = qzk_zd_shfl64(acc, 3);
    if (lane != 0) return;
    uint64_t h;
    if (stripes) {
        h = qzk_xx_rotl(acc, 1) + qzk_xx_rotl(a1, 7) + qzk_xx_rotl(a2, 12) + qzk_xx_rotl(a3, 18);
        h = qzk_xx_merge(h, acc); h = qzk_xx_merge(h, a1); h = qzk_xx_merge(h, a2); h = qzk_xx_merge(h, a3);
    } else h = QZK_XXP5;
    h += n;
    uint32_t i = stripes << 5;
    for (; i + 8 <= n; i += 8) h = qzk_xx_rotl(h ^ qzk_xx_round(0, qzk_rb_ld64(p + i)), 27) * QZK_XXP1 + QZK_XXP4;
    if (i + 4 <= n) { h = qzk_xx_rotl(h ^ ((uint64_t)qz_ld32(p + i) * QZK_XXP1), 23) * QZK_XXP2 + QZK_XXP3; i += 4; }
    for (; i < n; i++) h = qzk_xx_rotl(h ^ ((uint64_t)p[i] * QZK_XXP5), 11) * QZK_XXP1;
    h ^= h >> 33; h *= QZK_XXP2; h ^= h >> 29; h *= QZK_XXP3; h ^= h >> 32;
    if ((uint32_t)h != qz_ld32(in + rs.in_used - 4)) res[f].status = QZK_ZD_ECKSUM;
}

#endif
