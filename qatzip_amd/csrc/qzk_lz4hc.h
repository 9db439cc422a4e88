/*
 * qzk_lz4hc.h — LZ4-HC (liblz4 1.9.3 LZ4HC_compress_hashChain, compression levels 3-8) for gfx950, one wave per 64 KB block.
 *
 * Same place in the reference as K4 (LZ4F_compressFrame behind qzLZ4SWCompress, src/qatzip_sw.c:443-471): with
 * comp_lvl >= 3 liblz4 runs its hash-chain parser instead of the fast one.  What makes it different from the fast parser
 * for a GPU: LZ4HC_Insert puts EVERY position below a search point into the chains, and the search points of a block only
 * move forward, so the chains do not depend on the parse; and every block of a linked frame starts its parse afresh at
 * its first byte.  So all blocks of a call can be parsed at once, each by its own wave:
 *
 *   H1 qzk_lz4hc_chain_kernel   per block: for the 64 KB in front of the block (its history window, as far as the frame
 *                               reaches back) and the block itself, the distance from each position to the previous one
 *                               with the same hash of four bytes, capped at 65535 - what liblz4's chainTable holds for
 *                               that position, and what its hashTable answers when that position is searched
 *   H2 qzk_lz4hc_parse_kernel   per block: the parse itself (best match, the wider-match searches, the two- and
 *                               three-match overlap rules) into the block's slot, with the frame's header in front of a
 *                               frame's first block and room for its end mark and checksum behind the last one
 *      qzk_lz4hc_xxh_kernel     per frame: XXH32 of the content - one serial chain per frame, about a gigabyte a second,
 *                               so it runs beside H1 / H2 on a stream of its own and not behind them
 *   H3 qzk_lz4hc_finish_kernel  after the scan and the gather of the slots: end mark and content checksum into the stream
 *
 * Where the window lives: a block's history plus the block is 128 KB of input and 256 KB of chain distances.  Both are read
 * through the L2 and none of it is staged in LDS: the chains alone are more than a CU's 160 KiB, and the input alone
 * (128 KB) would leave one wave per CU, where this parse - one dependent load per chain hop, nothing to overlap it with
 * inside a wave - lives on the number of waves a CU keeps in flight.  The only LDS here is the content hash's 2 KiB of
 * staging, so the wave slots and not the LDS decide the occupancy.  Neither choice has been measured against the other.
 *
 * The control flow of a block is wave-uniform (liblz4's own, statement by statement); the lanes share the byte compares
 * of a candidate (256 bytes a trip) and the literal copies.
 *
 * Coordinates: a block works in positions relative to its window start `ws` (the block's start minus 64 KB, or the frame's
 * start), so they fit 17 bits and liblz4's lowLimit test (`index >= max(lowLimit, ip - 65535)`) keeps its form.
 */
#ifndef QZK_LZ4HC_H
#define QZK_LZ4HC_H
#include "qzk_lz4.h"

#define QZK_HC_HSIZE 32768u         /* LZ4HC_HASHTABLESIZE */
#define QZK_HC_MAXD 65535u          /* LZ4_DISTANCE_MAX: what a chainTable entry is capped at */
#define QZK_HC_OPTML 18             /* OPTIMAL_ML */
#define QZK_HC_WIN 131072u          /* chain distances per block: window + block */
#define QZK_HC_HDRMAX 15u
QZ_DEV uint32_t qzk_hc_hash(uint32_t v) { return (v * 2654435761u) >> 17; }

/* search attempts of a level (lz4hc.c clTable); 0 = not one of the hash-chain levels this header restates */
QZ_DEV int qzk_hc_attempts(int level) { return level >= 3 && level <= 8 ? 4 << (level - 3) : 0; }

/* where block g of the call lies: its frame, the frame's bytes, the block's bounds inside the frame */
typedef struct { uint32_t frame, k, flen, bs, be, last; uint64_t foff; } qzk_hc_geo;
QZ_DEV qzk_hc_geo qzk_hc_locate(uint64_t total, uint32_t frame_sz, uint32_t bpf, uint32_t g)
{
    qzk_hc_geo G;
    G.frame = g / bpf; G.k = g % bpf;
    G.foff = (uint64_t)G.frame * frame_sz;
    G.flen = total - G.foff < frame_sz ? (uint32_t)(total - G.foff) : frame_sz;
    G.bs = G.k * QZK_LZ4_MAXBLK;
    G.be = G.flen - G.bs < QZK_LZ4_MAXBLK ? G.flen : G.bs + QZK_LZ4_MAXBLK;
    G.last = G.be == G.flen;
    return G;
}

/* H1: one wave per block, 64 positions a trip (the grouping of qzk_lazy_chain_kernel: a position's predecessor is the
 * nearest earlier lane of the trip with its hash, else what the head table holds from earlier trips; the last lane of each
 * hash writes the table).  head_all: QZK_HC_HSIZE words per block of the launch, zeroed by the host, position + 1.
 * chain_all: QZK_HC_WIN entries per block, entry q - ws for position q.  A position without a predecessor in the frame
 * gets 65535, as in liblz4, whose cleared hashTable points 64 KB below the frame's start. */
QZ_KERNEL_MAX(64) qzk_lz4hc_chain_kernel(const uint8_t *src, uint64_t total, uint32_t frame_sz, uint32_t bpf, uint32_t g0,
                                         uint32_t nblocks, uint32_t *head_all, uint16_t *chain_all)
{
    if (blockIdx.x >= nblocks) return;
    const int lane = qz_lane();
    const qzk_hc_geo G = qzk_hc_locate(total, frame_sz, bpf, g0 + blockIdx.x);
    const uint32_t ws = G.bs >= QZK_LZ4_MAXBLK ? G.bs - QZK_LZ4_MAXBLK : 0;
    const uint8_t *in = src + G.foff + ws;
    const uint32_t n = G.be - ws, lim = G.flen - ws;                /* positions of this wave; bytes that may be read */
    uint32_t *head = head_all + (size_t)blockIdx.x * QZK_HC_HSIZE;
    uint16_t *ch = chain_all + (size_t)blockIdx.x * QZK_HC_WIN;
    for (uint32_t P0 = 0; P0 < n; P0 += 64) {
        const uint32_t p = P0 + (uint32_t)lane;
        const bool valid = p < n && p + 4 <= lim;
        uint32_t h = 0;
        if (valid) h = qzk_hc_hash(qz_ld32(in + p));
        int near = -1; bool later = false;
        uint64_t todo = qz_ballot(valid);
        while (todo) {
            const int j = qz_ctz64(todo);
            const uint32_t hj = qz_readlane(h, j);
            const uint64_t grp = qz_ballot(valid && h == hj);
            if ((grp >> lane) & 1) {
                const uint64_t below = grp & qz_below(lane);
                near = below ? qz_msb64(below) : -1;
                later = (grp >> lane) >> 1 != 0;
            }
            todo &= ~grp;
        }
        qz_wave_sync();                                 /* the previous trip's table stores are visible */
        uint32_t q1 = 0;                                /* predecessor's position + 1, 0 = none */
        if (valid) q1 = near >= 0 ? P0 + (uint32_t)near + 1 : head[h];
        if (valid) ch[p] = (uint16_t)((q1 != 0 && p + 1 - q1 < QZK_HC_MAXD) ? p + 1 - q1 : QZK_HC_MAXD);
        qz_wave_sync();                                 /* every lane has read the table before any lane writes it */
        if (valid && !later) head[h] = p + 1;
    }
}

/* LZ4HC_countBack: how far the match at (s, m) reaches back, s not below ilow, m not below the window's first byte;
 * returns the (positive) number of bytes */
QZ_DEV uint32_t qzk_hc_countback(const uint8_t *in, uint32_t s, uint32_t m, uint32_t ilow, int lane)
{
    const uint32_t maxb = s - ilow < m ? s - ilow : m;
    uint32_t back = 0;
    while (back < maxb) {
        const uint32_t i = back + 1 + (uint32_t)lane;
        const bool act = i <= maxb;
        const bool ne = act && in[s - i] != in[m - i];
        const uint64_t mm = qz_ballot(ne), am = qz_ballot(act);
        if (mm) { back += (uint32_t)qz_ctz64(mm); break; }
        back += (uint32_t)qz_popc64(am);
    }
    return back;
}

/* LZ4HC_InsertAndGetWiderMatch (prefix mode, no pattern analysis, no chain swap - the hash-chain levels below 9): the
 * longest match for the string at s that may start as early as ilow, among at most `attempts` candidates of s's chain;
 * `longest` comes in as the length to beat.  *mpos / *spos are written only when it is beaten. */
QZ_DEV int qzk_hc_search(const uint8_t *in, const uint16_t *ch, uint32_t s, uint32_t ilow, uint32_t mlimit, int longest,
                         uint32_t *mpos, uint32_t *spos, int attempts, int lane)
{
    const uint32_t lowest = s > QZK_HC_MAXD ? s - QZK_HC_MAXD : 0;
    const uint32_t lookback = s - ilow;
    const uint32_t pattern = qz_ld32(in + s);
    uint32_t d = ch[s];
    /* the first candidate is hashTable's: a capped distance stands for "exactly 65535" (a candidate), for something
     * farther and for nothing at all - the position 65535 back has the hash of s only in the first case */
    if (d == QZK_HC_MAXD && !(s >= QZK_HC_MAXD && qzk_hc_hash(qz_ld32(in + s - QZK_HC_MAXD)) == qzk_hc_hash(pattern))) return longest;
    uint32_t m = s - d;
    while (attempts > 0) {
        attempts--;
        const uint32_t nd = ch[m];                                  /* asked for before the compare that may not need it */
        if (qz_ld16(in + ilow + (uint32_t)longest - 1) == qz_ld16(in + m - lookback + (uint32_t)longest - 1) && qz_ld32(in + m) == pattern) {
            const uint32_t back = lookback ? qzk_hc_countback(in, s, m, ilow, lane) : 0;
            const int ml = 4 + (int)qzk_lz4_count(in + s + 4, in + m + 4, mlimit - (s + 4), lane) + (int)back;
            if (ml > longest) { longest = ml; *mpos = m - back; *spos = s - back; }
        }
        if (m < lowest + nd) break;                                 /* the next candidate lies below the lowest index */
        m -= nd;
    }
    return longest;
}

typedef struct { const uint8_t *in; uint8_t *out; uint32_t cap, op, ip, anchor; } qzk_hc_enc;
/* LZ4HC_encodeSequence with limitedOutput: true when the block does not fit */
QZ_DEV bool qzk_hc_encode(qzk_hc_enc *E, int ml, uint32_t ref, int lane)
{
    const uint32_t token_at = E->op++;
    uint32_t length = E->ip - E->anchor, tok;
    if (E->op + length / 255 + length + (2 + 1 + QZK_LZ4_LASTLIT) > E->cap) return true;
    if (length >= 15) {
        uint32_t len = length - 15; tok = 15u << 4;
        for (; len >= 255; len -= 255) { if (lane == 0) E->out[E->op] = 255; E->op++; }
        if (lane == 0) E->out[E->op] = (uint8_t)len;
        E->op++;
    } else tok = length << 4;
    qzk_wave_copy(E->out + E->op, E->in + E->anchor, length, lane); E->op += length;
    if (lane == 0) { E->out[E->op] = (uint8_t)(E->ip - ref); E->out[E->op + 1] = (uint8_t)((E->ip - ref) >> 8); }
    E->op += 2;
    length = (uint32_t)ml - QZK_LZ4_MINMATCH;
    if (E->op + length / 255 + (1 + QZK_LZ4_LASTLIT) > E->cap) return true;
    if (length >= 15) {
        tok += 15; length -= 15;
        for (; length >= 255; length -= 255) { if (lane == 0) E->out[E->op] = 255; E->op++; }
        if (lane == 0) E->out[E->op] = (uint8_t)length;
        E->op++;
    } else tok += length;
    if (lane == 0) E->out[token_at] = (uint8_t)tok;
    E->ip += (uint32_t)ml;
    E->anchor = E->ip;
    return false;
}

/* LZ4HC_compress_hashChain of in[bs..be) (window coordinates, chain distances in ch) into out with liblz4's
 * limitedOutput rules for a capacity of cap bytes; returns the block's size, 0 when it does not fit */
QZ_DEV uint32_t qzk_hc_block(const uint8_t *in, const uint16_t *ch, uint32_t bs, uint32_t be, uint8_t *out, uint32_t cap,
                             int attempts, int lane)
{
    qzk_hc_enc E; E.in = in; E.out = out; E.cap = cap; E.op = 0; E.ip = bs; E.anchor = bs;
    if (be - bs >= QZK_LZ4_MFLIMIT + 1) {
        const uint32_t mflimit = be - QZK_LZ4_MFLIMIT, matchlimit = be - QZK_LZ4_LASTLIT;
        int ml = 0, ml2 = 0, ml3 = 0, ml0 = 0;
        uint32_t ref = 0, ref2 = 0, ref3 = 0, ref0 = 0, start0 = 0, start2 = 0, start3 = 0;
        enum { MAIN, SEARCH2, SEARCH3 } st = MAIN;
        for (;;) {
            if (st == MAIN) {
                if (E.ip > mflimit) break;
                uint32_t unused = E.ip;
                ml = qzk_hc_search(in, ch, E.ip, E.ip, matchlimit, QZK_LZ4_MINMATCH - 1, &ref, &unused, attempts, lane);
                if (ml < QZK_LZ4_MINMATCH) { E.ip++; continue; }
                start0 = E.ip; ref0 = ref; ml0 = ml;                /* saved, in case we would skip too much */
                st = SEARCH2;
            }
            if (st == SEARCH2) {
                if (E.ip + (uint32_t)ml <= mflimit)
                    ml2 = qzk_hc_search(in, ch, E.ip + (uint32_t)ml - 2, E.ip, matchlimit, ml, &ref2, &start2, attempts, lane);
                else ml2 = ml;
                if (ml2 == ml) {                                    /* no better match: encode ML1 */
                    if (qzk_hc_encode(&E, ml, ref, lane)) return 0;
                    st = MAIN; continue;
                }
                if (start0 < E.ip && start2 < E.ip + (uint32_t)ml0) { E.ip = start0; ref = ref0; ml = ml0; }   /* squeezing ML1 between ML0 and ML2: restore */
                if (start2 - E.ip < 3) { ml = ml2; E.ip = start2; ref = ref2; continue; }   /* first match too small: removed */
                st = SEARCH3;
            }
            /* SEARCH3: ml2 > ml, and ip + 3 <= start2 */
            if (start2 - E.ip < QZK_HC_OPTML) {
                int new_ml = ml;
                if (new_ml > QZK_HC_OPTML) new_ml = QZK_HC_OPTML;
                if (E.ip + (uint32_t)new_ml > start2 + (uint32_t)ml2 - QZK_LZ4_MINMATCH) new_ml = (int)(start2 - E.ip) + ml2 - QZK_LZ4_MINMATCH;
                const int correction = new_ml - (int)(start2 - E.ip);
                if (correction > 0) { start2 += (uint32_t)correction; ref2 += (uint32_t)correction; ml2 -= correction; }
            }
            if (start2 + (uint32_t)ml2 <= mflimit)
                ml3 = qzk_hc_search(in, ch, start2 + (uint32_t)ml2 - 3, start2, matchlimit, ml2, &ref3, &start3, attempts, lane);
            else ml3 = ml2;
            if (ml3 == ml2) {                                       /* no better match: encode ML1 and ML2 */
                if (start2 < E.ip + (uint32_t)ml) ml = (int)(start2 - E.ip);
                if (qzk_hc_encode(&E, ml, ref, lane)) return 0;
                E.ip = start2;
                if (qzk_hc_encode(&E, ml2, ref2, lane)) return 0;
                st = MAIN; continue;
            }
            if (start3 < E.ip + (uint32_t)ml + 3) {                 /* not enough space for match 2: remove it */
                if (start3 >= E.ip + (uint32_t)ml) {                /* Seq1 can be written at once; Seq3 becomes Seq1 */
                    if (start2 < E.ip + (uint32_t)ml) {
                        const int correction = (int)(E.ip + (uint32_t)ml - start2);
                        start2 += (uint32_t)correction; ref2 += (uint32_t)correction; ml2 -= correction;
                        if (ml2 < QZK_LZ4_MINMATCH) { start2 = start3; ref2 = ref3; ml2 = ml3; }
                    }
                    if (qzk_hc_encode(&E, ml, ref, lane)) return 0;
                    E.ip = start3; ref = ref3; ml = ml3;
                    start0 = start2; ref0 = ref2; ml0 = ml2;
                    st = SEARCH2; continue;
                }
                start2 = start3; ref2 = ref3; ml2 = ml3;
                st = SEARCH3; continue;
            }
            /* three ascending matches: write the first one */
            if (start2 < E.ip + (uint32_t)ml) {
                if (start2 - E.ip < QZK_HC_OPTML) {
                    if (ml > QZK_HC_OPTML) ml = QZK_HC_OPTML;
                    if (E.ip + (uint32_t)ml > start2 + (uint32_t)ml2 - QZK_LZ4_MINMATCH) ml = (int)(start2 - E.ip) + ml2 - QZK_LZ4_MINMATCH;
                    const int correction = ml - (int)(start2 - E.ip);
                    if (correction > 0) { start2 += (uint32_t)correction; ref2 += (uint32_t)correction; ml2 -= correction; }
                } else ml = (int)(start2 - E.ip);
            }
            if (qzk_hc_encode(&E, ml, ref, lane)) return 0;
            E.ip = start2; ref = ref2; ml = ml2;                    /* ML2 becomes ML1 */
            start2 = start3; ref2 = ref3; ml2 = ml3;                /* ML3 becomes ML2 */
            st = SEARCH3;
        }
    }
    /* last literals */
    uint32_t op = E.op;
    const uint32_t lr = be - E.anchor;
    if (op + 1 + (lr + 255 - 15) / 255 + lr > cap) return 0;
    if (lr >= 15) {
        uint32_t acc = lr - 15;
        if (lane == 0) out[op] = 15u << 4;
        op++;
        for (; acc >= 255; acc -= 255) { if (lane == 0) out[op] = 255; op++; }
        if (lane == 0) out[op] = (uint8_t)acc;
        op++;
    } else { if (lane == 0) out[op] = (uint8_t)(lr << 4); op++; }
    qzk_wave_copy(out + op, in + E.anchor, lr, lane); op += lr;
    return op;
}

/* The frames' content checksums: one wave per frame.  XXH32 is one serial chain per frame (about a gigabyte a second), so
 * the device layer runs this beside H1 / H2 on a stream of its own, and H3 waits for it. */
QZ_KERNEL_MAX(64) qzk_lz4hc_xxh_kernel(const uint8_t *src, uint64_t total, uint32_t frame_sz, uint32_t nframes, uint32_t *xx)
{
    QZ_LDS __attribute__((aligned(16))) uint8_t stage[2048];       /* qzk_wave_xxh32_staged's stripes */
    const int lane = qz_lane();
    const uint32_t f = blockIdx.x;
    if (f >= nframes) return;
    const uint64_t foff = (uint64_t)f * frame_sz;
    const uint32_t flen = total - foff < frame_sz ? (uint32_t)(total - foff) : frame_sz;
    const uint32_t h = qzk_wave_xxh32_staged(src + foff, flen, stage, lane);
    if (lane == 0) xx[f] = h;
}

/* H2: workgroup i parses block g0 + i into slot i: [frame header, before a frame's first block][block word][block]
 * [eight bytes for the end mark and the content checksum, behind a frame's last block - written by H3].
 * hw_hdr: qzLZ4HeaderGen's header (FLG 0x4C whatever the size), as in qzk_lz4c_frame. */
QZ_KERNEL_MAX(64) qzk_lz4hc_parse_kernel(const uint8_t *src, uint64_t total, uint32_t frame_sz, uint32_t bpf, uint32_t g0,
                                         uint32_t nblocks, const uint16_t *chain_all, uint8_t *slots,
                                         uint32_t stride, uint32_t *lens, uint32_t hw_hdr, int attempts)
{
    const int lane = qz_lane();
    const uint32_t b = blockIdx.x;
    if (b >= nblocks) return;
    const qzk_hc_geo G = qzk_hc_locate(total, frame_sz, bpf, g0 + b);
    const uint32_t ws = G.bs >= QZK_LZ4_MAXBLK ? G.bs - QZK_LZ4_MAXBLK : 0;
    const uint8_t *in = src + G.foff + ws;
    uint8_t *o = slots + (size_t)b * stride;
    uint32_t pos = 0;
    if (G.k == 0) {
        const uint32_t n = G.flen;
        if (lane == 0) {
            o[0] = 0x04; o[1] = 0x22; o[2] = 0x4d; o[3] = 0x18;
            o[4] = hw_hdr ? (uint8_t)0x4C : (uint8_t)((1u << 6) | (n <= QZK_LZ4_MAXBLK ? 1u << 5 : 0) | (n ? 1u << 3 : 0) | (1u << 2));
            o[5] = 4u << 4;
            if (n || hw_hdr) { o[6] = (uint8_t)n; o[7] = (uint8_t)(n >> 8); o[8] = (uint8_t)(n >> 16); o[9] = (uint8_t)(n >> 24); o[10] = o[11] = o[12] = o[13] = 0; }
        }
        qz_wave_sync();
        pos = (n || hw_hdr) ? 14 : 6;
        const uint32_t hc = qzk_xxh32_small(o + 4, pos - 4);
        if (lane == 0) o[pos] = (uint8_t)(hc >> 8);
        pos++;
    }
    const uint32_t n = G.be - G.bs;
    if (n) {
        uint32_t c = qzk_hc_block(in, chain_all + (size_t)b * QZK_HC_WIN, G.bs - ws, G.be - ws, o + pos + 4, n - 1, attempts, lane);
        const uint32_t bh = c ? c : (n | 0x80000000u);
        if (c == 0) { qz_wave_sync(); qzk_wave_copy(o + pos + 4, in + (G.bs - ws), n, lane); c = n; }
        if (lane == 0) { o[pos] = (uint8_t)bh; o[pos + 1] = (uint8_t)(bh >> 8); o[pos + 2] = (uint8_t)(bh >> 16); o[pos + 3] = (uint8_t)(bh >> 24); }
        pos += 4 + c;
    }
    if (G.last) pos += 8;
    lens[b] = pos;                  /* wave-uniform: every lane stores the same word */
}

/* H3: one thread per frame that may end in the blocks [g0, g0 + nblocks) (the device layer: all of them, once the rounds and
 * the hashes are through): end mark and XXH32 of the content into the eight bytes its last block's slot kept free.
 * offs / lens: entry i for block g0 + i. */
QZ_KERNEL qzk_lz4hc_finish_kernel(uint64_t total, uint32_t frame_sz, uint32_t bpf, uint32_t g0, uint32_t nblocks, uint32_t nb_total,
                                  const uint64_t *offs, const uint32_t *lens, const uint32_t *xx, uint8_t *dst, uint64_t cap)
{
    const uint32_t f = g0 / bpf + blockIdx.x * blockDim.x + threadIdx.x;
    if ((uint64_t)f * bpf >= nb_total) return;
    const uint32_t lastb = (uint64_t)(f + 1) * bpf < nb_total ? (f + 1) * bpf - 1 : nb_total - 1;
    if (lastb < g0 || lastb >= g0 + nblocks) return;
    (void)total; (void)frame_sz;
    const uint64_t end = offs[lastb - g0] + lens[lastb - g0];
    if (end > cap) return;          /* (the gather has flagged it) */
    uint8_t *d = dst + end - 8;
    const uint32_t h = xx[f];
    d[0] = d[1] = d[2] = d[3] = 0;
    d[4] = (uint8_t)h; d[5] = (uint8_t)(h >> 8); d[6] = (uint8_t)(h >> 16); d[7] = (uint8_t)(h >> 24);
}

#endif
