/*
 * qzk_zstd_parse.h — Kzp: a hash-chain lazy parse for zstd sessions (include/qzamd_zstd_parse.h), gfx950, one wave per
 * hw_buff_sz chunk throughout.  K4s's parse (qzk_lz4s.h) is cut for LZ4s: one candidate a position, offsets to 65535, no
 * notion of a repeat offset.  This one feeds the same entropy stage (qzk_zstd.h: qzk_zs_frame) with sequences found the way
 * the lazy deflate levels (qzk_deflate_lazy.h) and LZ4-HC (qzk_lz4hc.h) find theirs, in stages that do not depend on one
 * another's decisions:
 *
 *   P1 qzk_zstd_chain_kernel   for every position of the chunk the distance to the previous position with the same hash of
 *                              mini_match bytes, 0 for none (qzk_lz4hc_chain_kernel's grouping: 64 positions a trip, the
 *                              nearest earlier lane with the hash, else the head table; the LAST lane of each hash writes
 *                              the table, so no store order decides anything)
 *   P2 qzk_zstd_search_kernel  64 consecutive positions at a time, each lane walking its own position's chain for at most
 *                              `depth` candidates: the longest match of at least mini_match bytes, the nearer one among
 *                              equals, any distance back to the chunk's start, any length up to the chunk's end.  A lane
 *                              counts QZK_ZP_LANECAP bytes on its own; a candidate that reaches the cap is finished by the
 *                              whole wave (256 bytes a trip, as K4s does).  A walk ends early only where nothing can beat
 *                              what it has: the match reaches the chunk's end.  {length, distance} per position, a function
 *                              of (chunk, mini_match, depth) alone
 *   P3 qzk_zstd_lazy_kernel    the lazy evaluation, serial per chunk, a lookup per step, and what depends on the parse: the
 *                              repeat offsets.  Records and literals as qzd_zstd_encode_frames_ex takes them
 *   P4 qzk_zstd_parse_encode_kernel / _seq_kernel   qzk_zs_frame on those records, without / with the sequence flags
 *
 * P2's shortcut for long matches.  Equal bytes at distance d from p0 to e mean a match of e - p bytes at distance d for
 * every p in between, so what the wave counted once is kept: QZK_ZP_RUNS entries {d, p0, e} in LDS, direct-mapped by a hash
 * of d.  A hit gives the exact length, so the table changes the time only, never an answer.  Without it a chunk of one byte
 * value, or of one short period, costs a count to the chunk's end per position and candidate.
 *
 * P3, at a parse point p with ll literals waiting: the candidates are the stored match and a match at each of the three
 * offsets that have a repeat code there (RFC 8878, 3.1.1.5: rep1, rep2, rep3 with ll > 0; rep2, rep3, rep1 - 1 with
 * ll == 0), the first mini_match bytes compared by every lane alike and the rest counted by the wave.  The price of a
 * candidate is zstd's own: gain = 4 * ml - floor(log2(offset value)), the offset value 1 .. 3 for a repeat code and
 * offset + 3 otherwise; the highest gain wins, the lower offset value among equals.  A stored match is a candidate from a
 * gain of QZK_ZP_MINGAIN on: below it (three bytes from more than 4 back, four from more than 124, ...) the literals are
 * cheaper - tried 8 .. 12 on the four ratio corpora, 10 gave the smallest sum.  Then the look-ahead: the best candidate
 * at p + 1 replaces it when its gain is more than 4 higher, and (depth >= QZK_ZP_LAZY2) the one at p + 2 when more than 7
 * higher; either restarts the look-ahead from the new point.  A match that is not a repeat is extended backwards over equal
 * bytes into the waiting literals.  The history then moves as the entropy stage moves it (qzk_zs_offset_values), so what
 * P3 prices as a repeat is coded as one under QZ_ZSTD_SEQ_REPEAT_OFFSETS; without that flag the same sequences cost their
 * plain offsets.  One record per match whatever its length (LZ4s's 65535 does not bind here).
 *
 * The head table has block_sz >> QZK_ZP_HSHIFT entries of 32 bits per chunk, position + 1, zeroed by the host.  A colliding
 * candidate costs a hop and nothing else; shifts 0 .. 3 differ by 0.1 % of the output at depth 4 and by bytes at depth 64
 * (Kzp).
 *
 * Scratch of a chunk (qzk_zp_carve; the host plan is qzd_zstd_parse_host.h): head table, chain distances (32 bits: a
 * distance reaches 131072 - mini_match, from the last position with mini_match bytes behind it to the chunk's first; a
 * length 131071), results (2 x 32 bits), literals, records, and 16 bytes for the two counts.
 * No wave waits for another; every loop is bounded by depth or by the chunk's length.
 */
#ifndef QZK_ZSTD_PARSE_H
#define QZK_ZSTD_PARSE_H
#include "qzk_zstd.h"

#define QZK_ZP_MAXDEPTH 256u
#define QZK_ZP_LANECAP 32u          /* bytes a lane counts on its own */
#ifndef QZK_ZP_HSHIFT
#define QZK_ZP_HSHIFT 2u            /* head table: block_sz >> 2 entries (shifts 0 .. 3 were tried) */
#endif
#ifndef QZK_ZP_LAZY2
#define QZK_ZP_LAZY2 64u            /* from this depth on the look-ahead is two positions (what it pays below) */
#endif
#ifndef QZK_ZP_MINGAIN
#define QZK_ZP_MINGAIN 10           /* a stored match is a candidate from this gain on */
#endif
#define QZK_ZP_RUNBITS 8u
#define QZK_ZP_RUNS (1u << QZK_ZP_RUNBITS)

typedef struct { uint32_t len, dist; } qzk_zp_res;      /* 0, 0: nothing of mini_match bytes or more */

/* block_sz is a power of two in 1 KB .. 128 KB: 8 .. 15 bits with the shift of 2 (host and device) */
#define QZK_ZP_HBITS(block_sz) (31u - (uint32_t)__builtin_clz((uint32_t)(block_sz)) - QZK_ZP_HSHIFT)
QZ_DEV uint32_t qzk_zp_hbits(uint32_t block_sz) { return QZK_ZP_HBITS(block_sz); }
QZ_DEV uint32_t qzk_zp_hash(uint32_t v, uint32_t mm, uint32_t hbits) { return ((mm == 3 ? v << 8 : v) * 2654435761u) >> (32 - hbits); }

/* a chunk's scratch, every part a multiple of 16 bytes (host and device) */
#define QZK_ZP_HEADB(block_sz) ((uint64_t)4u << QZK_ZP_HBITS(block_sz))
#define QZK_ZP_CHAINB(block_sz) ((uint64_t)(block_sz) * 4u)
#define QZK_ZP_RESB(block_sz) ((uint64_t)(block_sz) * 8u)
#define QZK_ZP_METAB 16u
#define QZK_ZP_CHUNKB(block_sz) (QZK_ZP_HEADB(block_sz) + QZK_ZP_CHAINB(block_sz) + QZK_ZP_RESB(block_sz) + QZK_ZS_WAVEB(block_sz) + QZK_ZP_METAB)

typedef struct { uint32_t *head, *chain; qzk_zp_res *res; uint8_t *lits; qzk_zs_seq *seqs; uint32_t *meta; } qzk_zp_mem;
QZ_DEV qzk_zp_mem qzk_zp_carve(uint8_t *scratch, uint32_t block_sz, uint32_t i)
{
    qzk_zp_mem m;
    uint8_t *p = scratch + (uint64_t)i * QZK_ZP_CHUNKB(block_sz);
    m.head = (uint32_t *)p; p += QZK_ZP_HEADB(block_sz);
    m.chain = (uint32_t *)p; p += QZK_ZP_CHAINB(block_sz);
    m.res = (qzk_zp_res *)p; p += QZK_ZP_RESB(block_sz);
    m.lits = p; p += QZK_ZS_LITB(block_sz);
    m.seqs = (qzk_zs_seq *)p;
    m.meta = (uint32_t *)(p + (QZK_ZS_WAVEB(block_sz) - QZK_ZS_LITB(block_sz)));
    return m;
}

/* chunk i of a launch over src[0..src_len) in chunks of block_sz */
QZ_DEV uint32_t qzk_zp_chunk_len(uint64_t src_len, uint32_t block_sz, uint32_t i)
{
    const uint64_t off = (uint64_t)i * block_sz;
    return (uint32_t)((src_len - off) < block_sz ? (src_len - off) : block_sz);
}

/* P1.  scratch: the launch's chunks back to back, the head tables zeroed */
QZ_KERNEL_MAX(64) qzk_zstd_chain_kernel(const uint8_t *src, uint64_t src_len, uint32_t block_sz, uint32_t nblocks, uint32_t mm,
                                        uint8_t *scratch)
{
    if (blockIdx.x >= nblocks) return;
    const int lane = qz_lane();
    const uint8_t *in = src + (uint64_t)blockIdx.x * block_sz;
    const uint32_t n = qzk_zp_chunk_len(src_len, block_sz, blockIdx.x), hbits = qzk_zp_hbits(block_sz);
    const qzk_zp_mem M = qzk_zp_carve(scratch, block_sz, blockIdx.x);
    for (uint32_t P0 = 0; P0 < n; P0 += 64) {
        const uint32_t p = P0 + (uint32_t)lane;
        const bool valid = p + mm <= n;
        uint32_t h = 0;
        if (valid) h = qzk_zp_hash(qzk_l4s_ld(in, n, p), mm, hbits);
        int near = -1; bool later = false;
        uint64_t todo = qz_ballot(valid);
        while (todo) {                                              /* todo loses at least its lowest bit a trip */
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
        if (valid) q1 = near >= 0 ? P0 + (uint32_t)near + 1 : M.head[h];
        if (p < n) M.chain[p] = q1 ? p + 1 - q1 : 0;
        qz_wave_sync();                                 /* every lane has read the table before any lane writes it */
        if (valid && !later) M.head[h] = p + 1;
    }
}

/* P2 */
QZ_KERNEL_MAX(64) qzk_zstd_search_kernel(const uint8_t *src, uint64_t src_len, uint32_t block_sz, uint32_t nblocks, uint32_t mm,
                                         uint32_t depth, uint8_t *scratch)
{
    QZ_LDS uint32_t run_d[QZK_ZP_RUNS], run_p[QZK_ZP_RUNS], run_e[QZK_ZP_RUNS];
    if (blockIdx.x >= nblocks) return;
    const int lane = qz_lane();
    const uint8_t *in = src + (uint64_t)blockIdx.x * block_sz;
    const uint32_t n = qzk_zp_chunk_len(src_len, block_sz, blockIdx.x);
    const qzk_zp_mem M = qzk_zp_carve(scratch, block_sz, blockIdx.x);
    for (uint32_t i = (uint32_t)lane; i < QZK_ZP_RUNS; i += 64) run_d[i] = 0;       /* 0 is no distance */
    qz_lds_sync();
    for (uint32_t P0 = 0; P0 < n; P0 += 64) {
        const uint32_t p = P0 + (uint32_t)lane;
        const bool valid = p + mm <= n;
        uint32_t v = 0, d = 0, best = 0, bd = 0, hops = 0;
        if (valid) { v = qzk_l4s_ld(in, n, p); d = M.chain[p]; }
        bool active = valid && d != 0;
        uint32_t cur = p - d;
        const uint32_t maxlen = valid ? n - p : 0;
        while (qz_ballot(active)) {                                 /* every active lane spends one of its `depth` hops a trip */
            uint32_t len = 0, nd = 0;
            if (active) {
                nd = M.chain[cur];                                  /* asked for before the compare that may not need it */
                /* cur < p and p + mm <= n: the four bytes at cur end at p + 3 <= n at the latest */
                const uint32_t x = v ^ qz_ld32(in + cur);
                if ((mm == 3 ? x << 8 : x) == 0) {
                    const uint32_t lim = maxlen < QZK_ZP_LANECAP ? maxlen : QZK_ZP_LANECAP;
                    bool go = true;
                    while (go && len + 4 <= lim) {
                        const uint32_t y = qz_ld32(in + p + len) ^ qz_ld32(in + cur + len);
                        if (y) { len += (uint32_t)qz_ctz32(y) >> 3; go = false; }
                        else len += 4;
                    }
                    while (go && len < lim && in[p + len] == in[cur + len]) len++;
                }
            }
            /* the candidates that reached the cap, one after the other, by the whole wave; not those that cannot pass what
             * the lane holds (best < maxlen here, so the byte behind it is the chunk's) */
            uint64_t m = qz_ballot(active && len >= QZK_ZP_LANECAP && len < maxlen &&
                                   (best < QZK_ZP_LANECAP || in[cur + best] == in[p + best]));
            while (m) {                                             /* m loses its lowest bit a trip */
                const int j = qz_ctz64(m);
                const uint32_t pj = qz_readlane(p, j), cj = qz_readlane(cur, j), dj = pj - cj;
                const uint32_t slot = (dj * 2654435761u) >> (32 - QZK_ZP_RUNBITS);
                const bool hit = run_d[slot] == dj && run_p[slot] <= pj && pj < run_e[slot];
                uint32_t e = run_e[slot];
                qz_lds_sync();                                      /* every lane has read the entry before lane 0 replaces it */
                if (!hit) {
                    e = pj + QZK_ZP_LANECAP + qzk_lz4_count(in + pj + QZK_ZP_LANECAP, in + cj + QZK_ZP_LANECAP, n - (pj + QZK_ZP_LANECAP), lane);
                    if (lane == 0) { run_d[slot] = dj; run_p[slot] = pj; run_e[slot] = e; }
                    qz_lds_sync();
                }
                if (lane == j) len = e - pj;
                m &= m - 1;
            }
            if (active) {
                if (len >= mm && len > best) { best = len; bd = p - cur; }
                hops++;
                /* a match to the chunk's end cannot be beaten, and what follows in the chain is farther away */
                if (best == maxlen || nd == 0 || hops >= depth) active = false;
                else cur -= nd;                                     /* nd <= cur: the chain points at a position of the chunk */
            }
        }
        if (p < n) { qzk_zp_res r; r.len = best; r.dist = bd; M.res[p] = r; }
    }
}

/* ------------------------------------------------------------------ P3 */
/* the offset value of `off` with ll literals in front, under the history r (the rule of qzk_zs_offset_values) */
QZ_DEV uint32_t qzk_zp_ov(uint32_t off, bool ll, const uint32_t *r)
{
    if (ll) return off == r[0] ? 1u : off == r[1] ? 2u : off == r[2] ? 3u : off + 3;
    return off == r[1] ? 1u : off == r[2] ? 2u : off == r[0] - 1 ? 3u : off + 3;
}
/* the history after a sequence of that offset value */
QZ_DEV void qzk_zp_push(uint32_t off, uint32_t ov, bool ll, uint32_t *r)
{
    if (ll && ov == 1) return;
    if ((ll && ov == 2) || (!ll && ov == 1)) { r[1] = r[0]; r[0] = off; return; }
    r[2] = r[1]; r[1] = r[0]; r[0] = off;
}

typedef struct { uint32_t ml, off, ov; int32_t gain; } qzk_zp_cand;

/* the best candidate at p with `ll` literals (or none) in front; ml == 0: there is none.  Wave-uniform. */
QZ_DEV qzk_zp_cand qzk_zp_best(const uint8_t *in, uint32_t n, uint32_t p, bool ll, const uint32_t *r, const qzk_zp_res *res,
                               uint32_t mm, int lane)
{
    qzk_zp_cand b; b.ml = 0; b.off = 0; b.ov = 0; b.gain = 0;
    const qzk_zp_res s = res[p];
    if (s.len >= mm) {
        const uint32_t ov = qzk_zp_ov(s.dist, ll, r);
        /* three bytes from far away cost more than three literals */
        if ((int32_t)(4 * s.len) - (int32_t)qzk_zs_hb(ov) >= (int32_t)QZK_ZP_MINGAIN) { b.ml = s.len; b.off = s.dist; b.ov = ov; b.gain = (int32_t)(4 * s.len) - (int32_t)qzk_zs_hb(ov); }
    }
    const uint32_t v = qzk_l4s_ld(in, n, p);
    for (uint32_t k = 0; k < 3; k++) {
        const uint32_t off = ll ? r[k] : k < 2 ? r[k + 1] : r[0] - 1;
        if (off == 0 || off > p || off == b.off) continue;
        /* p + mm <= n (the caller's), so the four bytes at p - off end inside the chunk */
        const uint32_t x = v ^ qz_ld32(in + p - off);
        if ((mm == 3 ? x << 8 : x) != 0) continue;
        const uint32_t ml = mm + qzk_lz4_count(in + p + mm, in + p - off + mm, n - (p + mm), lane);
        const uint32_t ov = qzk_zp_ov(off, ll, r);
        const int32_t gain = (int32_t)(4 * ml) - (int32_t)qzk_zs_hb(ov);
        if (b.ml == 0 || gain > b.gain || (gain == b.gain && ov < b.ov)) { b.ml = ml; b.off = off; b.ov = ov; b.gain = gain; }
    }
    return b;
}

/* the sequences of in[0..n) from the results of P2; returns the number of records, *nl_out = the literals */
QZ_DEV uint32_t qzk_zp_lazy(const uint8_t *in, uint32_t n, const qzk_zp_res *res, uint32_t mm, uint32_t depth, qzk_zs_seq *seqs,
                            uint8_t *lits, uint32_t *nl_out, int lane)
{
    uint32_t r[3] = { 1, 4, 8 };
    uint32_t p = 0, anchor = 0, ns = 0, nl = 0;
    while (p + mm <= n) {                                           /* p grows every trip */
        qzk_zp_cand c = qzk_zp_best(in, n, p, p > anchor, r, res, mm, lane);
        if (c.ml == 0) { p++; continue; }
        for (;;) {                                                  /* the look-ahead: p grows every trip */
            bool moved = false;
            for (uint32_t a = 1; a <= (depth >= QZK_ZP_LAZY2 ? 2u : 1u) && !moved; a++) {
                if (p + a + mm > n) break;
                const qzk_zp_cand c2 = qzk_zp_best(in, n, p + a, true, r, res, mm, lane);
                if (c2.ml && c2.gain > c.gain + (a == 1 ? 4 : 7)) { c = c2; p += a; moved = true; }
            }
            if (!moved) break;
        }
        if (c.ov > 3)                                               /* not a repeat: backwards over equal bytes */
            while (p > anchor && p > c.off && in[p - 1] == in[p - 1 - c.off]) { p--; c.ml++; }
        const uint32_t ll = p - anchor;
        c.ov = qzk_zp_ov(c.off, ll != 0, r);                       /* (the literals in front may have changed) */
        qzk_wave_copy(lits + nl, in + anchor, ll, lane);
        if (lane == 0) { seqs[ns].ll = ll; seqs[ns].ml = c.ml; seqs[ns].off = c.off; }
        qzk_zp_push(c.off, c.ov, ll != 0, r);
        nl += ll; ns++;
        p += c.ml; anchor = p;
    }
    if (anchor < n) { qzk_wave_copy(lits + nl, in + anchor, n - anchor, lane); nl += n - anchor; }
    *nl_out = nl;
    return ns;
}

QZ_KERNEL_MAX(64) qzk_zstd_lazy_kernel(const uint8_t *src, uint64_t src_len, uint32_t block_sz, uint32_t nblocks, uint32_t mm,
                                       uint32_t depth, uint8_t *scratch)
{
    if (blockIdx.x >= nblocks) return;
    const int lane = qz_lane();
    const uint8_t *in = src + (uint64_t)blockIdx.x * block_sz;
    const uint32_t n = qzk_zp_chunk_len(src_len, block_sz, blockIdx.x);
    const qzk_zp_mem M = qzk_zp_carve(scratch, block_sz, blockIdx.x);
    uint32_t nl = 0;
    const uint32_t ns = qzk_zp_lazy(in, n, M.res, mm, depth, M.seqs, M.lits, &nl, lane);
    if (lane == 0) { M.meta[0] = ns; M.meta[1] = nl; }
}

/* P4: persistent single-wave workgroups pull chunk numbers (as qzk_zstd_pull_kernel); chunk b's records become its frame in
 * slot b, out_len[b] = the frame's size.  With SEQ the offset values overwrite the records' offsets, as in qzk_zstd_pull. */
template <bool SEQ>
QZ_DEV void qzk_zstd_parse_encode(qzk_zs_lds *S, qzk_zs_xlds *X, const qzk_zs_tabs *T, const uint8_t *src, uint64_t src_len,
                                  uint32_t block_sz, uint32_t nblocks, uint8_t *slots, uint32_t stride, uint32_t *out_len,
                                  uint32_t *counter, uint8_t *scratch, uint32_t flags)
{
    const int lane = qz_lane();
    for (;;) {
        uint32_t b = atomicAdd(counter, lane == 0 ? 1u : 0u);
        b = qz_readfirstlane(b);
        if (b >= nblocks) break;
        const qzk_zp_mem M = qzk_zp_carve(scratch, block_sz, b);
        const uint32_t n = qzk_zp_chunk_len(src_len, block_sz, b);
        const uint32_t c = qzk_zs_frame<SEQ>(S, X, T, src + (uint64_t)b * block_sz, n, M.seqs, M.meta[0], &M.seqs[0].off, 3, flags,
                                             M.lits, M.meta[1], slots + (uint64_t)b * stride, lane);
        out_len[b] = c;                 /* wave-uniform: every lane stores the same word */
        qz_wave_sync();
    }
}
QZ_KERNEL_MAX(64) qzk_zstd_parse_encode_kernel(const uint8_t *src, uint64_t src_len, uint32_t block_sz, uint32_t nblocks, uint8_t *slots,
                                               uint32_t stride, uint32_t *out_len, uint32_t *counter, uint8_t *scratch)
{
    QZ_LDS uint32_t table[QZK_L4S_HSIZE];                           /* the stage's LDS, laid out as in qzk_zstd_pull_kernel */
    QZ_LDS qzk_zs_tabs T;
    qzk_zs_tabs_init(&T, qz_lane());
    qzk_zstd_parse_encode<false>((qzk_zs_lds *)table, NULL, &T, src, src_len, block_sz, nblocks, slots, stride, out_len, counter, scratch, 0);
}
QZ_KERNEL_MAX(64) qzk_zstd_parse_encode_seq_kernel(const uint8_t *src, uint64_t src_len, uint32_t block_sz, uint32_t nblocks, uint8_t *slots,
                                                   uint32_t stride, uint32_t *out_len, uint32_t *counter, uint8_t *scratch,
                                                   uint32_t seq_flags)
{
    QZ_LDS uint32_t table[QZK_L4S_HSIZE];
    QZ_LDS qzk_zs_tabs T;
    qzk_zs_tabs_init(&T, qz_lane());
    qzk_zstd_parse_encode<true>((qzk_zs_lds *)table, (qzk_zs_xlds *)((uint8_t *)table + QZK_ZS_XOFF), &T, src, src_len, block_sz, nblocks,
                                slots, stride, out_len, counter, scratch, seq_flags);
}

#endif
