/*
 * qzk_lz4s.h — K4s: LZ4s blocks (the LZ77 sequence format a QAT device hands to a post-processing callback; the consumer
 * is the reference's utils/qzstd.c:118-179, the per-chunk header src/qatzip_lz4.c:219-231) for gfx950, one wave per
 * hw_buff_sz chunk.
 *
 *   block    := u32le size, then `size` bytes of sequences
 *   sequence := token | [lit-len bytes] | literals | ( end of block | u16le offset | [match-len bytes] )
 *
 * token >> 4 is the literal length L, token & 15 the match code M, both extended by LZ4's 15 / 255 rule.  M == 0: no match,
 * the offset is written as 0; M > 0: a match of M + mini_match - 1 bytes, `offset` bytes back in this chunk.  No length
 * of one sequence passes 65535 (the consumer keeps them in 16 bits): longer literal runs go on in M == 0 sequences, longer
 * matches in further matches.  None of LZ4's end rules; no empty trailing sequence.
 *
 * The contract is the format, not a parse, so the parse is cut for 64 lanes instead of replaying a serial one (K4):
 *
 *   window   lane i owns position cur + i and hashes its four bytes; the bucket's entry - the LAST earlier position with
 *            that hash - is its candidate.  With mini_match 3 the three bytes are hashed as well, into the same table, and
 *            that bucket's entry is the candidate when the first does not hold: a three-byte hash alone finds the three-byte
 *            matches but too often the shorter of two candidates (text: 1.11 of liblz4's size instead of 1.06);
 *   insert   every position of the window goes into the table, in groups of QZK_L4S_GROUP lanes from the left: a group
 *            reads its entries, then inserts (atomicMax: the highest position wins whatever the order of the lanes' stores),
 *            then the next group reads.  So a candidate lies in an earlier group, never in the lane's own, and what the
 *            table holds depends on the chunk alone.  One group of 64 misses every match whose source is in the same
 *            window - runs, short periods: 4.8 times liblz4's size on `runs`; groups of 16 / 8 / 4: 1.95 / 1.44 / 1.12;
 *   count    each lane compares its own candidate, up to QZK_L4S_LANECAP bytes;
 *   pick     left to right by ballot: the first lane that has a match and is not beaten by the lane behind it (one step
 *            of lazy evaluation); a match that reached the lane cap is extended by the whole wave, 256 bytes a trip; the
 *            sequence is written (literals by all lanes), and the pick goes on behind the match;
 *   advance  cur moves to the end of the window or of the last match, whichever is farther.
 *
 * The table: QZK_L4S_HSIZE = 4096 entries of 32 bits in LDS, cleared per chunk.  LDS has no 16-bit atomic max, and the
 * winner of a bucket must not depend on store order, so the entries are words for every chunk size (positions up to 512 KB
 * fit); an empty entry is 0, which is position 0 - a candidate like any other, verified by comparing its bytes.  16 KiB per
 * wave leaves ten waves a CU (160 KiB).  2048 entries (twenty waves) put text at 1.14 and lzmix at 1.15 of liblz4's size,
 * above what tests/test_sim_lz4s.py allows; 8192 (five waves) reach 1.01 and 1.03.  That choice rests on the emulator's
 * ratios alone: no GPU rate has been taken at 2048 or 8192 entries, nor at another group width.
 *
 * Measured (profiles/lz4s_rates.txt: 1 GiB resident, 64 KB chunks, K4 25.9 GB/s in the same process): 27.4 GB/s with
 * mini_match 4, 24.4 with 3 - level with K4, not ahead of it; 128 KB chunks 23.2 / 20.6, 512 KB 14.7 / 13.1.  The counters
 * there: 61 % of the wave cycles waiting at 2.5 waves a SIMD, 3.3 scalar instructions per vector one (the serial pick-and-
 * write part), more store than load instructions.  Token, offset and length bytes are lane 0's byte stores straight to
 * global memory; K4's LDS staging (QZK_L4C_OST) for them is not used yet and is the first thing to try.
 *
 * The lazy step looks one lane ahead and is decided for all lanes before the picks: a lane that stepped back for a
 * successor which an earlier match then swallows does not get its own match back.
 * That costs ratio only (text: 1.06 of liblz4's level-1 size, 1.10 allowed).
 *
 * The bound (qzd_lz4s_bound): a sequence with a match is taken only when it is no longer than what it covers plus one byte
 * per 255 covered (qzk_l4s_parse, `the rule`), so all literals is the worst case.
 */
#ifndef QZK_LZ4S_H
#define QZK_LZ4S_H
#include "qzk_lz4.h"

#ifndef QZK_L4S_HBITS
#define QZK_L4S_HBITS 12
#endif
#define QZK_L4S_HSIZE (1u << QZK_L4S_HBITS)
#ifndef QZK_L4S_GROUP
#define QZK_L4S_GROUP 4u
#endif
#define QZK_L4S_LANECAP 32u         /* bytes a lane counts on its own */
#define QZK_L4S_MAXRUN 65535u       /* literals, and match bytes, of one sequence */
#define QZK_L4S_MAXOFF 65535u
#define QZK_L4S_MINBLK 1024u
#define QZK_L4S_MAXBLK 524288u

/* what a block of c input bytes can grow to, its size word included: c literals in runs of 65535 cost a token, 257 length
 * bytes and (all runs but the last) two offset bytes each - c + c/255 + 4 * ceil(c/65535) covers them; 16 to spare */
#define QZK_L4S_BOUND(c) (4u + (uint32_t)(c) + (uint32_t)(c) / 255u + 4u * (((uint32_t)(c) + 65534u) / 65535u) + 16u)   /* (host and device) */

QZ_DEV uint32_t qzk_l4s_hash(uint32_t v, uint32_t mm) { return ((mm == 3 ? v << 8 : v) * 2654435761u) >> (32 - QZK_L4S_HBITS); }

/* the four bytes at p of a chunk of n; bytes behind the chunk read as zero */
QZ_DEV uint32_t qzk_l4s_ld(const uint8_t *in, uint32_t n, uint32_t p)
{
    if (p + 4 <= n) return qz_ld32(in + p);
    uint32_t v = 0;
    for (uint32_t t = 0; t < 4; t++) if (p + t < n) v |= (uint32_t)in[p + t] << (8 * t);
    return v;
}

/* v in bytes of 255 (a length that did not fit its nibble, less 15) */
QZ_DEV uint32_t qzk_l4s_len(uint8_t *out, uint32_t op, uint32_t v, int lane)
{
    const uint32_t nff = v / 255u;
    for (uint32_t i = (uint32_t)lane; i < nff; i += 64) out[op + i] = 255;
    if (lane == 0) out[op + nff] = (uint8_t)(v - 255u * nff);
    return op + nff + 1;
}

/* one sequence: L literals from lit, then the block's end (end: M == 0) or the offset and the match code M */
QZ_DEV uint32_t qzk_l4s_put(uint8_t *out, uint32_t op, const uint8_t *lit, uint32_t L, uint32_t M, uint32_t off, bool end, int lane)
{
    if (lane == 0) out[op] = (uint8_t)(((L < 15 ? L : 15u) << 4) | (M < 15 ? M : 15u));
    op++;
    if (L >= 15) op = qzk_l4s_len(out, op, L - 15, lane);
    qzk_wave_copy(out + op, lit, L, lane);
    op += L;
    if (end) return op;
    if (lane == 0) { out[op] = (uint8_t)off; out[op + 1] = (uint8_t)(off >> 8); }
    op += 2;
    if (M >= 15) op = qzk_l4s_len(out, op, M - 15, lane);
    return op;
}

/* L literals from lit and a match of ml >= mm bytes, in as many sequences as the 16-bit lengths ask for */
QZ_DEV uint32_t qzk_l4s_seq(uint8_t *out, uint32_t op, const uint8_t *lit, uint32_t L, uint32_t off, uint32_t ml, uint32_t mm, int lane)
{
    while (L > QZK_L4S_MAXRUN) { op = qzk_l4s_put(out, op, lit, QZK_L4S_MAXRUN, 0, 0, false, lane); lit += QZK_L4S_MAXRUN; L -= QZK_L4S_MAXRUN; }
    while (ml) {
        /* a piece of 65535 bytes, unless that would leave less than a match behind it */
        uint32_t take = ml;
        if (ml > QZK_L4S_MAXRUN) take = ml - QZK_L4S_MAXRUN < mm ? QZK_L4S_MAXRUN - mm : QZK_L4S_MAXRUN;
        op = qzk_l4s_put(out, op, lit, L, take - mm + 1, off, false, lane);
        L = 0; ml -= take;
    }
    return op;
}

/* the L >= 1 literals a block ends with */
QZ_DEV uint32_t qzk_l4s_tail(uint8_t *out, uint32_t op, const uint8_t *lit, uint32_t L, int lane)
{
    while (L > QZK_L4S_MAXRUN) { op = qzk_l4s_put(out, op, lit, QZK_L4S_MAXRUN, 0, 0, false, lane); lit += QZK_L4S_MAXRUN; L -= QZK_L4S_MAXRUN; }
    return qzk_l4s_put(out, op, lit, L, 0, 0, true, lane);
}

/* what the parse hands its sequences to.  This one writes the LZ4s bytes; qzk_zstd.h has a second one, which keeps
 * (literal length, match length, offset) records and the literal bytes for the zstd entropy stage.  An emitter E has
 * qzk_l4s_emit(E &, lit, L, off, ml, mm, lane) - L literals and a match of ml >= mm bytes - and
 * qzk_l4s_emit_tail(E &, lit, L, lane) - the L >= 1 literals a chunk ends with; both are called by the whole wave with
 * wave-uniform arguments.  What the parse decides never depends on the emitter. */
typedef struct { uint8_t *out; uint32_t op; } qzk_l4s_bytes;
QZ_DEV void qzk_l4s_emit(qzk_l4s_bytes &e, const uint8_t *lit, uint32_t L, uint32_t off, uint32_t ml, uint32_t mm, int lane)
{
    e.op = qzk_l4s_seq(e.out, e.op, lit, L, off, ml, mm, lane);
}
QZ_DEV void qzk_l4s_emit_tail(qzk_l4s_bytes &e, const uint8_t *lit, uint32_t L, int lane) { e.op = qzk_l4s_tail(e.out, e.op, lit, L, lane); }

/* the sequences of in[0..n), n >= 1, to the emitter; table: QZK_L4S_HSIZE words of LDS */
template <typename E>
QZ_DEV void qzk_l4s_parse(const uint8_t *in, uint32_t n, E &emit, uint32_t mm, uint32_t *table, int lane)
{
    for (uint32_t i = (uint32_t)lane; i < QZK_L4S_HSIZE; i += 64) table[i] = 0;
    qz_lds_sync();
    uint32_t cur = 0, anchor = 0;
    while (cur < n) {                                               /* cur grows by at least 64 a trip */
        const uint32_t p = cur + (uint32_t)lane;
        const bool valid = p + mm <= n;
        uint32_t v = 0, h = 0, h3 = 0, cand = 0, cand3 = 0, len = 0;
        if (valid) { v = qzk_l4s_ld(in, n, p); h = qzk_l4s_hash(v, 4); h3 = qzk_l4s_hash(v, 3); }
        for (uint32_t g = 0; g < 64; g += QZK_L4S_GROUP) {
            const bool mine = valid && ((uint32_t)lane & ~(QZK_L4S_GROUP - 1)) == g;
            if (mine) { cand = table[h]; if (mm == 3) cand3 = table[h3]; }
            qz_lds_sync();                                          /* the group has read the table before any of its lanes writes it */
            if (mine) { atomicMax(&table[h], p); if (mm == 3) atomicMax(&table[h3], p); }
            qz_lds_sync();
        }
        /* the candidate of the four-byte hash if it holds, else (mini_match 3) the one of the three-byte hash.
         * cand < p, so cand + 4 <= p + 3 <= n; the window: nothing farther back than 65535 */
        if (mm == 3 && !(valid && cand < p && p - cand <= QZK_L4S_MAXOFF && qz_ld32(in + cand) == v)) cand = cand3;
        if (valid && cand < p && p - cand <= QZK_L4S_MAXOFF) {
            const uint32_t x = v ^ qz_ld32(in + cand);
            if ((mm == 3 ? x << 8 : x) == 0) {
                const uint32_t lim = n - p < QZK_L4S_LANECAP ? n - p : QZK_L4S_LANECAP;
                bool go = true;
                while (go && len + 4 <= lim) {
                    const uint32_t y = qz_ld32(in + p + len) ^ qz_ld32(in + cand + len);
                    if (y) { len += (uint32_t)qz_ctz32(y) >> 3; go = false; }
                    else len += 4;
                }
                while (go && len < lim && in[p + len] == in[cand + len]) len++;
            }
        }
        /* one step of lazy evaluation: a lane steps back when the position behind it has the longer match */
        const uint32_t nlen = qz_shfl(len, lane + 1);
        uint64_t m = qz_ballot(len >= mm && !(lane < 63 && nlen > len));
        while (m) {                                                 /* m loses at least its lowest bit a trip */
            const int j = qz_ctz64(m);
            uint32_t ml = qz_readlane(len, j);
            const uint32_t c = qz_readlane(cand, j), pj = cur + (uint32_t)j;
            /* the rule behind the bound: token, offset and the match's length bytes are fewer than the match's bytes from
             * four bytes on, with one to spare for the literals' first length byte; a match of three pays for token and
             * offset only, so it is taken when the literals before it still fit the token (mini_match 3 only) */
            if (ml == 3 && pj - anchor >= 15) { m &= m - 1; continue; }
            if (ml >= QZK_L4S_LANECAP) ml += qzk_lz4_count(in + pj + ml, in + c + ml, n - (pj + ml), lane);
            qzk_l4s_emit(emit, in + anchor, pj - anchor, pj - c, ml, mm, lane);
            anchor = pj + ml;
            const uint32_t nx = (uint32_t)j + ml;
            m = nx >= 64 ? 0 : m & ~qz_below((int)nx);
        }
        cur = anchor > cur + 64 ? anchor : cur + 64;
    }
    if (anchor < n) qzk_l4s_emit_tail(emit, in + anchor, n - anchor, lane);
}

/* the sequences of in[0..n), n >= 1, as LZ4s bytes into out (QZK_L4S_BOUND(n) - 4 bytes are enough); returns their size */
QZ_DEV uint32_t qzk_l4s_block(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t mm, uint32_t *table, int lane)
{
    qzk_l4s_bytes e = { out, 0 };
    qzk_l4s_parse(in, n, e, mm, table, lane);
    return e.op;
}

/* K4s: persistent single-wave workgroups pull chunk numbers (as qzk_lz4c_pull_kernel); chunk b of the launch goes to slot b
 * as [size word][sequences], out_len[b] = 4 + size.  No wave waits for another. */
QZ_KERNEL_MAX(64) qzk_lz4s_pull_kernel(const uint8_t *src, uint64_t src_len, uint32_t block_sz, uint32_t nblocks, uint8_t *slots,
                                       uint32_t stride, uint32_t *out_len, uint32_t mm, uint32_t *counter)
{
    QZ_LDS uint32_t table[QZK_L4S_HSIZE];
    const int lane = qz_lane();
    for (;;) {
        uint32_t b = atomicAdd(counter, lane == 0 ? 1u : 0u);        /* every lane takes part, lane 0 adds */
        b = qz_readfirstlane(b);
        if (b >= nblocks) break;
        const uint64_t off = (uint64_t)b * block_sz;
        const uint32_t n = (uint32_t)((src_len - off) < block_sz ? (src_len - off) : block_sz);
        uint8_t *o = slots + (uint64_t)b * stride;
        const uint32_t c = qzk_l4s_block(src + off, n, o + 4, mm, table, lane);
        if (lane == 0) { o[0] = (uint8_t)c; o[1] = (uint8_t)(c >> 8); o[2] = (uint8_t)(c >> 16); o[3] = (uint8_t)(c >> 24); }
        out_len[b] = c + 4;             /* wave-uniform: every lane stores the same word */
        qz_wave_sync();
    }
}

#endif
