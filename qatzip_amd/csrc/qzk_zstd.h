/*
 * qzk_zstd.h — Kz: zstd frames (RFC 8878) for gfx950, one wave per hw_buff_sz chunk: K4s's parse (qzk_lz4s.h) with a record
 * emitter, then the entropy stage.  What the reference reaches with a CPU callback (utils/qzstd.c:118-279: decLz4Block,
 * then libzstd's ZSTD_compressSequences, one frame per chunk) is here one kernel.
 *
 *   frame    := 28 B5 2F FD | descriptor (Single_Segment, no dictionary id, no checksum) | Frame_Content_Size in 1, 2 or 4
 *               bytes, the smallest that holds the chunk | ONE block with Last_Block set
 *   block    := Compressed when that is strictly smaller than the chunk, Raw otherwise
 *   literals := the smallest of Raw, RLE (every literal the same byte) and Compressed (a Huffman code of at most 11 bits
 *               built per block; its description direct 4-bit weights when the highest symbol is at most 128, FSE-compressed
 *               weights otherwise; one stream up to 1023 literals, four above); on equal sizes Raw, then RLE
 *   sequences:= count in 1, 2 or 3 bytes | modes | per RLE table its code | the backward bitstream.  Each of LL, OF, ML is
 *               RLE_Mode when every sequence has the same code and Predefined_Mode otherwise.  The offset value is always
 *               offset + 3: no repeat offsets.
 *   sequences, with seq_flags (qzamd_zstd_seq.h; the _seq kernels, qzk_zs_sequences_x):
 *               count | modes | per table in LL, OF, ML order nothing, its one code, or its description | the bitstream.
 *               QZK_ZS_SEQ_REP: the offset value comes from the repeat-offset history (RFC 8878, 3.1.1.5), 1, 4, 8 at the
 *               frame's start: with a literal length above 0, rep1 / rep2 / rep3 are 1 / 2 / 3; with a literal length of 0,
 *               rep2 / rep3 / rep1 - 1 are 1 / 2 / 3 and an offset equal to rep1 is offset + 3; the lowest value that fits.
 *               QZK_ZS_SEQ_FSE: a table that is not RLE is Predefined or FSE_Compressed, whichever takes fewer bits by an
 *               exact count (state bits of the whole chain, the final state, the description's bytes), Predefined on a
 *               tie.  Accuracy: log2(ns - 1) - 2 kept in 5 .. 9 (offsets 5 .. 8), and at least log2 of the codes present,
 *               rounded up.  Counts: count * 2^accuracy / ns rounded to nearest, at least 1 for a code that occurs; what
 *               the sum lacks goes to the most frequent code, what it has too much is taken from the then most frequent
 *               one at a time, the lower code among equals; no "less than one" entries.
 *
 * Not written: Repeat_Mode tables, treeless literals, more than one block, dictionaries, checksums.
 *
 * The record emitter follows decLz4Block's rule: the literals of an M == 0 sequence join the next sequence (so a literal
 * length can pass 65535: LL code 35), a match cut into pieces gives one record per piece, and the literals a chunk ends with
 * are in the literals section only.
 *
 * The stage, for one chunk (records and literals in global scratch of the wave, tables in LDS):
 *   literals   histogram by LDS atomics; the present symbols sorted by rank counting (a lane per four symbols); the tree by
 *              the two-queue method, the limit to 11 bits by moving leaves between the length counts (Kraft sum kept at
 *              one), lengths dealt out by frequency - lane 0, a few hundred steps; codes from the weights as the RFC's
 *              4.2.1.3 orders them; the streams packed 64 symbols a trip: prefix sum of the code lengths, atomicOr into a
 *              staging area in LDS, whole bytes out.  A stream is read backwards, so the LAST symbol goes to bit 0 and the
 *              closing 1-bit behind the first;
 *   sequences  codes and extra bits per lane; the LL, OF and ML state chains depend on nothing but themselves, so lanes 0, 1
 *              and 2 walk one each over the 64 sequences of a trip and leave (bits, count) per sequence in LDS; then every
 *              lane puts its sequence together - OF, ML, LL state bits, LL, ML, OF extra bits - and the same packer places
 *              them.  The stream is written from the last sequence to the first, the three final states and the 1-bit last.
 * Nothing is written past its limit (qzk_zs_bw::cap): a sequences section that would make the block as large as the chunk
 * stops being stored and the block becomes Raw.
 *
 * The predefined distributions (RFC 8878, 3.1.1.3.2.2.1-3), from which qzk_zs_tabs_init builds the encoding tables:
 *   literals lengths, accuracy 6: 4 3 2 2 2 2 2 2 2 2 2 2 2 1 1 1 2 2 2 2 2 2 2 2 2 3 2 1 1 1 1 1 -1 -1 -1 -1
 *   offsets, accuracy 5:          1 1 1 1 1 1 2 2 2 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 -1 -1 -1 -1 -1
 *   match lengths, accuracy 6:    1 4 3 2 2 2 2 2 2 1 (x37 ones from code 9 to 45) -1 -1 -1 -1 -1 -1 -1
 * and the codes (3.1.1.3.2.1.1): literal lengths 0-15 are their own code, then baselines 16 18 20 22 24 28 32 40 48 64 128 ...
 * 65536 with 1 1 1 1 2 2 3 3 4 6 7 ... 16 extra bits; match lengths 3-34 are codes 0-31, then baselines 35 37 39 41 43 47 51
 * 59 67 83 99 131 259 ... 65539 with 1 1 1 1 2 2 3 3 4 4 5 7 8 ... 16 extra bits; an offset value v has code floor(log2 v)
 * and that many extra bits.
 *
 * LDS: the stage's working set (qzk_zs_lds, 7.5 KiB) lies over the parse's table, which is dead by then; the three predefined
 * tables (qzk_zs_tabs, 1.7 KiB) are built once per wave and live beside it: 17.7 KiB a wave, nine waves a CU (K4s: ten).
 * With seq_flags a chunk's own tables and the stage's further scratch (qzk_zs_xlds, 6.5 KiB) lie behind qzk_zs_lds in the
 * same 16 KiB: the wave's LDS does not grow.  The stage then runs five passes over the records: offset values (the history
 * is serial: a trip of 64 records in the lanes' registers, read one by one), the three histograms by LDS atomics, a table plan per lane
 * 0-2, the cost walk (lanes 0-2 in the chunk's tables, 3-5 in the predefined ones), and the bitstream as above.
 */
#ifndef QZK_ZSTD_H
#define QZK_ZSTD_H
#include "qzk_lz4s.h"

#define QZK_ZS_MAXBLK 131072u       /* the reference's MAX_BLOCK_SIZE: one block per frame */
#define QZK_ZS_HUFLOG 11u
#define QZK_ZS_BOUND(c) ((uint32_t)(c) + 12u)       /* magic 4, descriptor 1, content size 4, block header 3 (host and device) */
#define QZK_ZS_SLACK 64u            /* what a slot has behind the bound: a literals section is tried up to 5 bytes past Raw's */
#define QZK_ZS_STAGEW 140u          /* words of the packer's staging area: 7 bits carried + 64 x 66 bits, two words to spare */
#define QZK_ZS_OVER 0xffffffffu

typedef struct { uint32_t ll, ml, off; } qzk_zs_seq;        /* literal length, match length (>= 3), offset (>= 1) */
typedef struct { uint64_t lit0, seq0; uint32_t content, nseq, nlit, pad; } qzk_zs_fdesc;   /* a frame of qzk_zstd_encode_kernel */

QZ_CONST int8_t QZK_ZS_LL_NORM[36] = { 4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1,
                                       -1, -1, -1, -1 };
QZ_CONST int8_t QZK_ZS_OF_NORM[29] = { 1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1 };
QZ_CONST int8_t QZK_ZS_ML_NORM[53] = { 1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                       1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1 };
QZ_CONST uint8_t QZK_ZS_LL_BITS[36] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12,
                                        13, 14, 15, 16 };
QZ_CONST uint8_t QZK_ZS_ML_BITS[53] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                        1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16 };
/* the code of a literal length below 64, and of a match length less 3 below 128 */
QZ_CONST uint8_t QZK_ZS_LL_CODE[64] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16, 17, 17, 18, 18, 19, 19,
                                        20, 20, 20, 20, 21, 21, 21, 21, 22, 22, 22, 22, 22, 22, 22, 22, 23, 23, 23, 23, 23, 23, 23, 23,
                                        24, 24, 24, 24, 24, 24, 24, 24, 24, 24, 24, 24, 24, 24, 24, 24 };
QZ_CONST uint8_t QZK_ZS_ML_CODE[128] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27,
                                         28, 29, 30, 31, 32, 32, 33, 33, 34, 34, 35, 35, 36, 36, 36, 36, 37, 37, 37, 37,
                                         38, 38, 38, 38, 38, 38, 38, 38, 39, 39, 39, 39, 39, 39, 39, 39,
                                         40, 40, 40, 40, 40, 40, 40, 40, 40, 40, 40, 40, 40, 40, 40, 40,
                                         41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41,
                                         42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42,
                                         42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42, 42 };

QZ_DEV uint32_t qzk_zs_hb(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }      /* v != 0 */
QZ_DEV uint32_t qzk_zs_ll_code(uint32_t ll) { return ll < 64 ? QZK_ZS_LL_CODE[ll] : qzk_zs_hb(ll) + 19; }
QZ_DEV uint32_t qzk_zs_ml_code(uint32_t mlb) { return mlb < 128 ? QZK_ZS_ML_CODE[mlb] : qzk_zs_hb(mlb) + 36; }

/* ------------------------------------------------------------------ the record emitter of K4s's parse */
typedef struct { qzk_zs_seq *seqs; uint8_t *lits; uint32_t ns, nl; } qzk_zs_rec;

/* the pieces of a match are qzk_l4s_seq's: what decLz4Block makes of the LZ4s bytes is then this list */
QZ_DEV void qzk_l4s_emit(qzk_zs_rec &e, const uint8_t *lit, uint32_t L, uint32_t off, uint32_t ml, uint32_t mm, int lane)
{
    qzk_wave_copy(e.lits + e.nl, lit, L, lane);
    e.nl += L;
    while (ml) {
        uint32_t take = ml;
        if (ml > QZK_L4S_MAXRUN) take = ml - QZK_L4S_MAXRUN < mm ? QZK_L4S_MAXRUN - mm : QZK_L4S_MAXRUN;
        if (lane == 0) { e.seqs[e.ns].ll = L; e.seqs[e.ns].ml = take; e.seqs[e.ns].off = off; }
        e.ns++;
        L = 0; ml -= take;
    }
}
QZ_DEV void qzk_l4s_emit_tail(qzk_zs_rec &e, const uint8_t *lit, uint32_t L, int lane)
{
    qzk_wave_copy(e.lits + e.nl, lit, L, lane);
    e.nl += L;
}

/* ------------------------------------------------------------------ FSE encoding tables */
/* a state is kept as table size + index.  Coding symbol s from state x: nb = (x + dnb[s]) >> 16 low bits of x go out,
 * the next state is st[(x >> nb) + dfs[s]].  Serial: run by one lane.  cnt: nsym entries of scratch, spread: 1 << log.
 * N and C hold a count and a position of the table: int8_t and uint8_t up to accuracy 6, int16_t and uint16_t above. */
template <typename N, typename C>
QZ_DEV void qzk_zs_fse_build(const N *norm, uint32_t nsym, uint32_t log, uint16_t *st, uint32_t *dnb, int32_t *dfs,
                             uint8_t *spread, C *cnt)
{
    const uint32_t size = 1u << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint32_t high = size - 1, pos = 0, total = 0;
    for (uint32_t s = 0; s < nsym; s++) if (norm[s] == -1) spread[high--] = (uint8_t)s;        /* "less than one": the table's end */
    for (uint32_t s = 0; s < nsym; s++)
        for (int i = 0; i < norm[s]; i++) {
            spread[pos] = (uint8_t)s;
            do pos = (pos + step) & mask; while (pos > high);
        }
    for (uint32_t s = 0; s < nsym; s++) {
        const int n = norm[s];
        cnt[s] = (C)total;                                          /* where the symbol's states begin in st */
        if (n == 0) { dnb[s] = ((log + 1) << 16) - size; dfs[s] = 0; }
        else if (n == -1 || n == 1) { dnb[s] = (log << 16) - size; dfs[s] = (int32_t)total - 1; total++; }
        else {
            const uint32_t maxbits = log - qzk_zs_hb((uint32_t)n - 1);
            dnb[s] = (maxbits << 16) - ((uint32_t)n << maxbits);
            dfs[s] = (int32_t)total - n;
            total += (uint32_t)n;
        }
    }
    for (uint32_t u = 0; u < size; u++) st[cnt[spread[u]]++] = (uint16_t)(size + u);
}
QZ_DEV uint32_t qzk_zs_fse_init(const uint16_t *st, const uint32_t *dnb, const int32_t *dfs, uint32_t s)
{
    const uint32_t nb = (dnb[s] + (1u << 15)) >> 16, v = (nb << 16) - dnb[s];
    return st[(int32_t)(v >> nb) + dfs[s]];
}

#define QZK_ZS_LL 0
#define QZK_ZS_OF 1
#define QZK_ZS_ML 2
/* the three predefined tables; table t has its states at st + ST0(t), its symbols at dnb/dfs + SY0(t) */
typedef struct {
    uint16_t st[160];
    uint32_t dnb[128]; int32_t dfs[128];
    uint8_t spread[3][64], cnt[3][64];
} qzk_zs_tabs;
#define QZK_ZS_ST0(t) ((t) == 0 ? 0u : (t) == 1 ? 64u : 96u)
#define QZK_ZS_SY0(t) ((t) == 0 ? 0u : (t) == 1 ? 36u : 68u)
#define QZK_ZS_LOG(t) ((t) == 1 ? 5u : 6u)

QZ_DEV void qzk_zs_tabs_init(qzk_zs_tabs *T, int lane)
{
    if (lane < 3) {
        const int8_t *norm = lane == 0 ? QZK_ZS_LL_NORM : lane == 1 ? QZK_ZS_OF_NORM : QZK_ZS_ML_NORM;
        qzk_zs_fse_build(norm, lane == 0 ? 36u : lane == 1 ? 29u : 53u, QZK_ZS_LOG(lane), T->st + QZK_ZS_ST0(lane),
                         T->dnb + QZK_ZS_SY0(lane), T->dfs + QZK_ZS_SY0(lane), T->spread[lane], T->cnt[lane]);
    }
    qz_lds_sync();
}

/* ------------------------------------------------------------------ the stage's LDS */
typedef struct {
    uint32_t hist[256];
    uint32_t ncnt[512];             /* tree: the leaves by rising count, then the inner nodes as they are made */
    uint16_t parent[512];
    uint16_t hcode[256];
    uint8_t depth[512];
    uint8_t hlen[256], sorted[256], weight[256];
    uint8_t desc[256];              /* the tree description */
    uint32_t stage[QZK_ZS_STAGEW];
    uint16_t wst[64]; uint32_t wdnb[16]; int32_t wdfs[16]; uint8_t wspread[64], wcnt[16]; int8_t wnorm[16];
    uint8_t code[3][64], sbits[3][64], snb[3][64];
    uint32_t v[4];                  /* lane 0 to the wave: [0] bytes of the description (0: there is none), [1] longest code */
} qzk_zs_lds;

static_assert(sizeof(qzk_zs_lds) <= 4 * QZK_L4S_HSIZE, "the stage's LDS lies over the parse's table");

QZ_DEV uint32_t qzk_zs_sum(uint32_t v) { return qz_readlane(qz_wave_incl_scan(v), 63); }

/* ------------------------------------------------------------------ the packer */
/* bytes go to out[op..]; `carry` holds the nbits < 8 bits that do not fill a byte yet.  Nothing is stored at or past cap:
 * `over` is set instead and op goes on counting. */
typedef struct { uint8_t *out; uint32_t op, cap, nbits, carry, over; } qzk_zs_bw;

QZ_DEV void qzk_zs_or_bits(uint32_t *stage, uint32_t pos, uint64_t v, uint32_t n)
{
    if (!n) return;
    v &= n >= 64 ? ~0ull : (1ull << n) - 1;
    const uint32_t w = pos >> 5, sh = pos & 31;
    const uint32_t lo = (uint32_t)(v << sh);
    const uint64_t hi = sh ? v >> (32 - sh) : v >> 32;
    if (lo) atomicOr(&stage[w], lo);
    if ((uint32_t)hi) atomicOr(&stage[w + 1], (uint32_t)hi);
    if (hi >> 32) atomicOr(&stage[w + 2], (uint32_t)(hi >> 32));
}

/* every lane's a (na bits) then b (nb bits), lane 0's first; na + nb <= 66, na and nb below 64 */
QZ_DEV void qzk_zs_pack(qzk_zs_lds *S, qzk_zs_bw *w, uint64_t a, uint32_t na, uint64_t b, uint32_t nb, int lane)
{
    const uint32_t incl = qz_wave_incl_scan(na + nb), all = qz_readlane(incl, 63);
    const uint32_t T = w->nbits + all, words = (T + 31) / 32 + 2, nbytes = T >> 3;
    for (uint32_t i = (uint32_t)lane; i < words; i += 64) S->stage[i] = 0;
    qz_lds_sync();
    if (lane == 0 && w->nbits) atomicOr(&S->stage[0], w->carry);
    const uint32_t pos = w->nbits + incl - (na + nb);
    qzk_zs_or_bits(S->stage, pos, a, na);
    qzk_zs_or_bits(S->stage, pos + na, b, nb);
    qz_lds_sync();
    if (w->op + nbytes <= w->cap)
        for (uint32_t i = (uint32_t)lane; i < nbytes; i += 64) w->out[w->op + i] = (uint8_t)(S->stage[i >> 2] >> (8 * (i & 3)));
    else w->over = 1;
    w->carry = (S->stage[nbytes >> 2] >> (8 * (nbytes & 3))) & 0xffu;
    w->op += nbytes; w->nbits = T & 7;
    qz_lds_sync();
}
/* the byte that is not full, if there is one; returns the stream's size */
QZ_DEV uint32_t qzk_zs_close(qzk_zs_bw *w, int lane)
{
    if (w->nbits) {
        if (w->op + 1 <= w->cap) { if (lane == 0) w->out[w->op] = (uint8_t)w->carry; }
        else w->over = 1;
        w->op++; w->nbits = 0;
    }
    return w->op;
}

/* ------------------------------------------------------------------ literals */
/* the histogram of lits[0..nl) into S->hist; returns the number of distinct bytes, *top = the highest of them */
QZ_DEV uint32_t qzk_zs_histogram(qzk_zs_lds *S, const uint8_t *lits, uint32_t nl, uint32_t *top, int lane)
{
    for (uint32_t i = (uint32_t)lane; i < 256; i += 64) S->hist[i] = 0;
    qz_lds_sync();
    for (uint32_t i = 4 * (uint32_t)lane; i + 4 <= nl; i += 256) {
        const uint32_t v = qz_ld32(lits + i);
        atomicAdd(&S->hist[v & 255], 1u); atomicAdd(&S->hist[(v >> 8) & 255], 1u);
        atomicAdd(&S->hist[(v >> 16) & 255], 1u); atomicAdd(&S->hist[v >> 24], 1u);
    }
    if ((uint32_t)lane < (nl & 3)) atomicAdd(&S->hist[lits[(nl & ~3u) + (uint32_t)lane]], 1u);
    qz_lds_sync();
    uint32_t m = 0;
    *top = 0;
    for (uint32_t k = 0; k < 4; k++) {
        const uint64_t b = qz_ballot(S->hist[64 * k + (uint32_t)lane] != 0);
        if (b) { m += (uint32_t)qz_popc64(b); *top = 64 * k + (uint32_t)qz_msb64(b); }
    }
    return m;
}

/* the tree description as FSE-compressed weights (RFC 8878, 4.2.1.2) of weight[0..nw) into S->desc, size byte first;
 * returns its size, 0 when there is none (one weight value only, or more than 127 bytes).  Lane 0 alone. */
QZ_DEV uint32_t qzk_zs_weights_fse(qzk_zs_lds *S, uint32_t nw)
{
    uint32_t cnt[13], nsym = 0, present = 0;
    for (uint32_t s = 0; s < 13; s++) cnt[s] = 0;
    for (uint32_t i = 0; i < nw; i++) cnt[S->weight[i]]++;
    for (uint32_t s = 0; s < 13; s++) if (cnt[s]) { nsym = s + 1; present++; }
    if (present < 2) return 0;
    /* normalised to 64: every present weight at least 1, the rounding error to (or from) the most frequent ones */
    const uint32_t log = 6, size = 64;
    int32_t sum = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        int32_t n = cnt[s] ? (int32_t)(cnt[s] * size / nw) : 0;
        if (cnt[s] && n == 0) n = 1;
        S->wnorm[s] = (int8_t)n; sum += n;
    }
    while (sum != (int32_t)size) {
        uint32_t best = 0;
        for (uint32_t s = 1; s < nsym; s++) if (S->wnorm[s] > S->wnorm[best]) best = s;
        if (sum < (int32_t)size) { S->wnorm[best] = (int8_t)(S->wnorm[best] + ((int32_t)size - sum)); sum = (int32_t)size; }
        else { S->wnorm[best]--; sum--; }                           /* the largest is above 1 while the sum is above 64 >= 13 */
    }
    /* the distribution (4.1.1): accuracy less 5 in four bits, then each value + 1 in as many bits as what remains asks for,
     * a value of 0 followed by a 2-bit count of further zeros */
    uint32_t dp = 1;
    uint64_t acc = log - 5; uint32_t nacc = 4;
    int32_t remaining = (int32_t)size + 1, threshold = (int32_t)size; uint32_t nbits = log + 1;
    uint32_t s = 0; bool prev0 = false;
    while (s < nsym && remaining > 1) {
        if (prev0) {
            uint32_t start = s;
            while (s < nsym && !S->wnorm[s]) s++;
            while (s >= start + 3) { start += 3; acc |= 3ull << nacc; nacc += 2; }     /* 13 symbols: never 24 zeros in a row */
            acc |= (uint64_t)(s - start) << nacc; nacc += 2;
        }
        int32_t c = S->wnorm[s++];
        const int32_t max = (2 * threshold - 1) - remaining;
        remaining -= c;
        c++;
        if (c >= threshold) c += max;
        acc |= (uint64_t)c << nacc; nacc += nbits;
        if (c < max) nacc--;
        prev0 = c == 1;
        while (remaining < threshold) { nbits--; threshold >>= 1; }
        while (nacc >= 8) { S->desc[dp++] = (uint8_t)acc; acc >>= 8; nacc -= 8; }
    }
    if (nacc) { S->desc[dp++] = (uint8_t)acc; }
    qzk_zs_fse_build(S->wnorm, nsym, log, S->wst, S->wdnb, S->wdfs, S->wspread, S->wcnt);
    /* two states take turns, the first weight on state one; written from the last weight back */
    uint32_t x[2] = { 0, 0 }; bool started[2] = { false, false };
    acc = 0; nacc = 0;
    for (uint32_t i = nw; i-- > 0;) {
        const uint32_t k = i & 1, sym = S->weight[i];
        if (!started[k]) { x[k] = qzk_zs_fse_init(S->wst, S->wdnb, S->wdfs, sym); started[k] = true; continue; }
        const uint32_t nb = (x[k] + S->wdnb[sym]) >> 16;
        acc |= (uint64_t)(x[k] & ((1u << nb) - 1)) << nacc; nacc += nb;
        x[k] = S->wst[(int32_t)(x[k] >> nb) + S->wdfs[sym]];
        while (nacc >= 8) { if (dp < 200) S->desc[dp] = (uint8_t)acc; dp++; acc >>= 8; nacc -= 8; }
    }
    acc |= (uint64_t)(x[1] & (size - 1)) << nacc; nacc += log;
    acc |= (uint64_t)(x[0] & (size - 1)) << nacc; nacc += log;
    acc |= 1ull << nacc; nacc++;
    while (nacc > 0) { if (dp < 200) S->desc[dp] = (uint8_t)acc; dp++; acc >>= 8; nacc = nacc >= 8 ? nacc - 8 : 0; }
    if (dp - 1 > 127) return 0;
    S->desc[0] = (uint8_t)(dp - 1);
    return dp;
}

/* a code of at most 11 bits for S->hist (m >= 2 distinct bytes, the highest `top`): S->hlen, S->hcode, S->desc.  Returns
 * the description's size, 0 when it cannot be written; *bits = what the literals take in this code. */
QZ_DEV uint32_t qzk_zs_huffman(qzk_zs_lds *S, uint32_t m, uint32_t top, uint32_t *bits, int lane)
{
    /* S->sorted: the present symbols by falling count, the lower symbol first among equals; a lane ranks four symbols */
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t s = 64 * k + (uint32_t)lane, c = S->hist[s];
        S->hlen[s] = 0; S->hcode[s] = 0;
        if (c) {
            uint32_t r = 0;
            for (uint32_t t = 0; t < 256; t++) { const uint32_t d = S->hist[t]; r += (d > c || (d == c && t < s)) ? 1u : 0u; }
            S->sorted[r] = (uint8_t)s;
        }
    }
    qz_lds_sync();
    if (lane == 0) {
        /* the tree, two queues: leaf i is sorted[m - 1 - i], the inner nodes m .. 2m - 2 come out by rising count too */
        for (uint32_t i = 0; i < m; i++) S->ncnt[i] = S->hist[S->sorted[m - 1 - i]];
        uint32_t lf = 0, in = m;
        for (uint32_t nn = m; nn < 2 * m - 1; nn++) {
            uint32_t pick[2];
            for (uint32_t q = 0; q < 2; q++) {
                if (lf < m && (in >= nn || S->ncnt[lf] <= S->ncnt[in])) pick[q] = lf++;
                else pick[q] = in++;
            }
            S->ncnt[nn] = S->ncnt[pick[0]] + S->ncnt[pick[1]];
            S->parent[pick[0]] = (uint16_t)nn; S->parent[pick[1]] = (uint16_t)nn;
        }
        uint32_t nc[QZK_ZS_HUFLOG + 1];
        for (uint32_t l = 0; l <= QZK_ZS_HUFLOG; l++) nc[l] = 0;
        S->depth[2 * m - 2] = 0;
        for (uint32_t k = 2 * m - 2; k-- > 0;) {
            const uint32_t d = (uint32_t)S->depth[S->parent[k]] + 1;
            S->depth[k] = (uint8_t)(d > 255 ? 255 : d);
            if (k < m) nc[d > QZK_ZS_HUFLOG ? QZK_ZS_HUFLOG : d]++;
        }
        /* the limit: the leaves that were deeper sit at 11 now, which overfills the code; take one from 11, and one from the
         * next shorter length that has any becomes two one level down - until the Kraft sum is one again */
        uint32_t total = 0;
        for (uint32_t l = 1; l <= QZK_ZS_HUFLOG; l++) total += nc[l] << (QZK_ZS_HUFLOG - l);
        while (total != (1u << QZK_ZS_HUFLOG)) {
            nc[QZK_ZS_HUFLOG]--;
            for (uint32_t l = QZK_ZS_HUFLOG - 1; l > 0; l--) if (nc[l]) { nc[l]--; nc[l + 1] += 2; break; }
            total--;
        }
        /* the shortest codes to the most frequent symbols */
        uint32_t maxbits = 0, idx = 0;
        for (uint32_t l = 1; l <= QZK_ZS_HUFLOG; l++)
            for (uint32_t k = 0; k < nc[l]; k++) { S->hlen[S->sorted[idx++]] = (uint8_t)l; maxbits = l; }
        /* codes (4.2.1.3): by rising weight, so from the longest codes on, counting from 0; in a weight by rising symbol */
        uint32_t next[QZK_ZS_HUFLOG + 2], code = 0;
        for (uint32_t l = maxbits; l >= 1; l--) { next[l] = code; code = (code + nc[l]) >> 1; }
        for (uint32_t s = 0; s <= top; s++) {
            const uint32_t l = S->hlen[s];
            if (l) S->hcode[s] = (uint16_t)next[l]++;
            S->weight[s] = (uint8_t)(l ? maxbits + 1 - l : 0);
        }
        /* the description covers symbols 0 .. top - 1: the last weight follows from the others */
        uint32_t dn;
        if (top <= 128) {
            S->desc[0] = (uint8_t)(127 + top);
            for (uint32_t i = 0; i < top; i += 2) S->desc[1 + i / 2] = (uint8_t)(S->weight[i] << 4 | (i + 1 < top ? S->weight[i + 1] : 0));
            dn = 1 + (top + 1) / 2;
        } else dn = qzk_zs_weights_fse(S, top);
        S->v[0] = dn; S->v[1] = maxbits;
    }
    qz_lds_sync();
    uint32_t b = 0;
    for (uint32_t k = 0; k < 4; k++) b += S->hist[64 * k + (uint32_t)lane] * S->hlen[64 * k + (uint32_t)lane];
    *bits = qzk_zs_sum(b);
    return S->v[0];
}

/* one Huffman stream of the m >= 1 literals at lits: the last symbol first, the 1-bit behind the first symbol */
QZ_DEV uint32_t qzk_zs_hstream(qzk_zs_lds *S, const uint8_t *lits, uint32_t m, uint8_t *out, uint32_t cap, int lane)
{
    qzk_zs_bw w = { out, 0, cap, 0, 0, 0 };
    for (uint32_t base = 0; base < m; base += 64) {
        const uint32_t j = base + (uint32_t)lane;
        uint32_t a = 0, na = 0;
        if (j < m) { const uint32_t sym = lits[m - 1 - j]; a = S->hcode[sym]; na = S->hlen[sym]; }
        qzk_zs_pack(S, &w, a, na, 0, 0, lane);
    }
    qzk_zs_pack(S, &w, lane == 0 ? 1u : 0u, lane == 0 ? 1u : 0u, 0, 0, lane);
    return qzk_zs_close(&w, lane);
}

QZ_DEV void qzk_zs_put_le(uint8_t *out, uint64_t v, uint32_t nbytes, int lane)
{
    if ((uint32_t)lane < nbytes) out[lane] = (uint8_t)(v >> (8 * lane));
}

/* the literals section of lits[0..nl) at out; returns its size, at most nl + 3.  Up to nl + 8 bytes are written. */
QZ_DEV uint32_t qzk_zs_literals(qzk_zs_lds *S, const uint8_t *lits, uint32_t nl, uint8_t *out, int lane)
{
    const uint32_t rh = nl < 32 ? 1u : nl < 4096 ? 2u : 3u, rawsz = rh + nl;
    const uint32_t fmt = rh == 1 ? 0u : rh == 2 ? 1u : 3u;
    uint32_t top = 0;
    const uint32_t m = nl ? qzk_zs_histogram(S, lits, nl, &top, lane) : 0;
    if (m == 1 && rh + 1 < rawsz) {                                 /* RLE */
        qzk_zs_put_le(out, 1u | fmt << 2 | (uint64_t)nl << (rh == 1 ? 3 : 4), rh, lane);
        if (lane == 0) out[rh] = lits[0];
        return rh + 1;
    }
    if (m >= 2) {
        uint32_t bits = 0;
        const uint32_t dn = qzk_zs_huffman(S, m, top, &bits, lane);
        const uint32_t ch = nl < 1024 ? 3u : nl < 16384 ? 4u : 5u, nst = nl < 1024 ? 1u : 4u, jt = nst == 4 ? 6u : 0u;
        /* the streams take bits / 8 + nst bytes at most, and at most nst - 1 fewer */
        if (dn && ch + dn + jt + (bits >> 3) + 1 < rawsz) {
            uint8_t *p = out + ch;
            for (uint32_t i = (uint32_t)lane; i < dn; i += 64) p[i] = S->desc[i];
            uint32_t csz = dn + jt;
            const uint32_t cap = nl + 8 - ch;                       /* of the section's data: nothing is stored past out + nl + 8 */
            if (nst == 1) csz += qzk_zs_hstream(S, lits, nl, p + csz, cap > csz ? cap - csz : 0, lane);
            else {
                const uint32_t seg = (nl + 3) / 4;
                uint64_t jump = 0;
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t from = k * seg, cnt = k < 3 ? seg : nl - 3 * seg;
                    const uint32_t sz = qzk_zs_hstream(S, lits + from, cnt, p + csz, cap > csz ? cap - csz : 0, lane);
                    if (k < 3) jump |= (uint64_t)(sz & 0xffffu) << (16 * k);
                    csz += sz;
                }
                qzk_zs_put_le(p + dn, jump, 6, lane);
            }
            if (ch + csz < rawsz) {
                const uint64_t h = 2u | (ch == 3 ? 0u : ch == 4 ? 2u : 3u) << 2 | (uint64_t)nl << 4 | (uint64_t)csz << (ch == 3 ? 14 : ch == 4 ? 18 : 22);
                qzk_zs_put_le(out, h, ch, lane);
                return ch + csz;
            }
            qz_wave_sync();                                         /* Raw goes over what was tried */
        }
    }
    qzk_zs_put_le(out, 0u | fmt << 2 | (uint64_t)nl << (rh == 1 ? 3 : 4), rh, lane);
    qzk_wave_copy(out + rh, lits, nl, lane);
    return rawsz;
}

/* ------------------------------------------------------------------ sequences */
/* the codes and extra bits of one record */
typedef struct { uint32_t llc, ofc, mlc, llx, ofx, mlx; } qzk_zs_codes;
QZ_DEV qzk_zs_codes qzk_zs_code_v(uint32_t ll, uint32_t ml, uint32_t ov)       /* ov: the offset value, 1 .. 3 a repeat code */
{
    qzk_zs_codes c;
    const uint32_t mlb = ml - 3;
    c.llc = qzk_zs_ll_code(ll); c.mlc = qzk_zs_ml_code(mlb); c.ofc = qzk_zs_hb(ov);
    c.llx = ll & ((1u << QZK_ZS_LL_BITS[c.llc]) - 1);
    c.mlx = mlb & ((1u << QZK_ZS_ML_BITS[c.mlc]) - 1);
    c.ofx = ov & ((1u << c.ofc) - 1);
    return c;
}
QZ_DEV qzk_zs_codes qzk_zs_code(const qzk_zs_seq q) { return qzk_zs_code_v(q.ll, q.ml, q.off + 3); }

/* the sequences section of seqs[0..ns) at out, where `cap` bytes may be stored; returns its size, QZK_ZS_OVER when it does
 * not fit.  Records as qzk_zs_check leaves them: ml >= 3, 1 <= off, all at most 128 KB. */
QZ_DEV uint32_t qzk_zs_sequences(qzk_zs_lds *S, const qzk_zs_tabs *T, const qzk_zs_seq *seqs, uint32_t ns, uint8_t *out, uint32_t cap,
                                 int lane)
{
    if (cap < 8) return QZK_ZS_OVER;
    if (ns == 0) { if (lane == 0) out[0] = 0; return 1; }
    uint32_t op;
    if (ns < 128) { if (lane == 0) out[0] = (uint8_t)ns; op = 1; }
    else if (ns < 0x7f00) { if (lane == 0) { out[0] = (uint8_t)((ns >> 8) + 128); out[1] = (uint8_t)ns; } op = 2; }
    else { if (lane == 0) { out[0] = 255; out[1] = (uint8_t)(ns - 0x7f00); out[2] = (uint8_t)((ns - 0x7f00) >> 8); } op = 3; }
    /* the modes: a table is RLE when no sequence has another code than the first one's */
    const qzk_zs_codes c0 = qzk_zs_code(seqs[0]);
    uint32_t differ = 0;
    for (uint32_t i = (uint32_t)lane; i < ns; i += 64) {
        const qzk_zs_codes c = qzk_zs_code(seqs[i]);
        differ |= (c.llc != c0.llc ? 1u : 0u) | (c.ofc != c0.ofc ? 2u : 0u) | (c.mlc != c0.mlc ? 4u : 0u);
    }
    const bool rle_ll = !qz_ballot(differ & 1), rle_of = !qz_ballot(differ & 2), rle_ml = !qz_ballot(differ & 4);
    if (lane == 0) {
        out[op] = (uint8_t)((rle_ll ? 1u : 0u) << 6 | (rle_of ? 1u : 0u) << 4 | (rle_ml ? 1u : 0u) << 2);
        uint32_t q = op + 1;
        if (rle_ll) out[q++] = (uint8_t)c0.llc;
        if (rle_of) out[q++] = (uint8_t)c0.ofc;
        if (rle_ml) out[q++] = (uint8_t)c0.mlc;
    }
    op += 1 + (rle_ll ? 1u : 0u) + (rle_of ? 1u : 0u) + (rle_ml ? 1u : 0u);
    /* lanes 0, 1, 2 own the LL, OF, ML chain */
    const bool myrle = lane == 0 ? rle_ll : lane == 1 ? rle_of : rle_ml;
    const int tl = lane < 3 ? lane : 0;
    const uint16_t *st = T->st + QZK_ZS_ST0(tl);
    const uint32_t *dnb = T->dnb + QZK_ZS_SY0(tl);
    const int32_t *dfs = T->dfs + QZK_ZS_SY0(tl);
    uint32_t x = 0;
    qzk_zs_bw w = { out + op, 0, cap - op, 0, 0, 0 };
    for (uint32_t base = 0; base < ns; base += 64) {                /* trip by trip from the last sequence back */
        const uint32_t j = base + (uint32_t)lane, cnt = ns - base < 64 ? ns - base : 64;
        qzk_zs_codes c = { 0, 0, 0, 0, 0, 0 };
        if (j < ns) c = qzk_zs_code(seqs[ns - 1 - j]);
        S->code[QZK_ZS_LL][lane] = (uint8_t)c.llc; S->code[QZK_ZS_OF][lane] = (uint8_t)c.ofc; S->code[QZK_ZS_ML][lane] = (uint8_t)c.mlc;
        qz_lds_sync();
        if (lane < 3) {
            for (uint32_t t = 0; t < cnt; t++) {
                uint32_t v = 0, nb = 0;
                if (!myrle) {
                    const uint32_t s = S->code[lane][t];
                    if (base + t == 0) x = qzk_zs_fse_init(st, dnb, dfs, s);
                    else {
                        nb = (x + dnb[s]) >> 16;
                        v = x & ((1u << nb) - 1);
                        x = st[(int32_t)(x >> nb) + dfs[s]];
                    }
                }
                S->sbits[lane][t] = (uint8_t)v; S->snb[lane][t] = (uint8_t)nb;
            }
        }
        qz_lds_sync();
        uint64_t a = 0, b = 0; uint32_t na = 0, nb = 0;
        if (j < ns) {
            a = S->sbits[QZK_ZS_OF][lane]; na = S->snb[QZK_ZS_OF][lane];
            a |= (uint64_t)S->sbits[QZK_ZS_ML][lane] << na; na += S->snb[QZK_ZS_ML][lane];
            a |= (uint64_t)S->sbits[QZK_ZS_LL][lane] << na; na += S->snb[QZK_ZS_LL][lane];
            a |= (uint64_t)c.llx << na; na += QZK_ZS_LL_BITS[c.llc];
            b = c.mlx; nb = QZK_ZS_ML_BITS[c.mlc];
            b |= (uint64_t)c.ofx << nb; nb += c.ofc;
        }
        qzk_zs_pack(S, &w, a, na, b, nb, lane);
    }
    /* the final states: ML, OF, LL, then the closing bit */
    const uint32_t xl = qz_readlane(x, 0), xo = qz_readlane(x, 1), xm = qz_readlane(x, 2);
    uint64_t a = 0; uint32_t na = 0;
    if (lane == 0) {
        if (!rle_ml) { a |= (uint64_t)(xm & 63u) << na; na += 6; }
        if (!rle_of) { a |= (uint64_t)(xo & 31u) << na; na += 5; }
        if (!rle_ll) { a |= (uint64_t)(xl & 63u) << na; na += 6; }
        a |= 1ull << na; na++;
    }
    qzk_zs_pack(S, &w, a, na, 0, 0, lane);
    qzk_zs_close(&w, lane);
    return w.over ? QZK_ZS_OVER : op + w.op;
}

/* ------------------------------------------------------------------ sequences, with chosen tables and repeat offsets */
#define QZK_ZS_SEQ_FSE 1u           /* QZ_ZSTD_SEQ_FSE_TABLES */
#define QZK_ZS_SEQ_REP 2u           /* QZ_ZSTD_SEQ_REPEAT_OFFSETS */
#define QZK_ZS_XST0(t) ((t) == 0 ? 0u : (t) == 1 ? 512u : 768u)
#define QZK_ZS_MAXLOG(t) ((t) == 1 ? 8u : 9u)
#define QZK_ZS_NSYM(t) ((t) == 0 ? 36u : (t) == 1 ? 32u : 53u)
#define QZK_ZS_OF_PREDEF 29u        /* the codes the predefined offset distribution has */
#define QZK_ZS_DESCB 96u            /* a description: 4 + 53 x 10 bits and at most 86 bits of zero runs are 78 bytes */

/* a chunk's own tables, symbols at SY0(t) as in qzk_zs_tabs, states at XST0(t); what lanes 0-2 leave for the wave */
typedef struct {
    uint16_t st[1280];
    uint32_t dnb[128]; int32_t dfs[128];
    uint8_t spread[1280];
    uint16_t cnt[128]; int16_t norm[128];
    uint32_t hist[128];
    uint16_t sbits[3][64];
    uint8_t desc[3][QZK_ZS_DESCB];
    uint32_t log[3], dsz[3], mode[3], top[3], cost[6];      /* mode: 0 Predefined, 1 RLE, 2 FSE_Compressed; top: the highest code */
} qzk_zs_xlds;
#define QZK_ZS_XOFF ((sizeof(qzk_zs_lds) + 15u) & ~(size_t)15u)
static_assert(QZK_ZS_XOFF + sizeof(qzk_zs_xlds) <= 4 * QZK_L4S_HSIZE, "a chunk's tables lie in what the stage leaves of the parse's table");

/* the offset values of seqs[0..ns) to ofv[i * ofs].  Without `rep` offset + 3.  With it the history of RFC 8878, 3.1.1.5,
 * which starts at 1, 4, 8: a literal length above 0 has rep1, rep2, rep3 for the values 1, 2, 3; a literal length of 0 has
 * rep2, rep3 and rep1 - 1 (an offset equal to rep1 has no repeat code then), the lowest value where several fit.  The
 * recurrence is serial, but it needs no lane: a trip of 64 records sits in the lanes' registers, the wave reads them one by
 * one (readlane: the record and the history are wave-uniform, the compares scalar) and the record's lane keeps the value.
 * ofv may be the records' own off fields. */
QZ_DEV void qzk_zs_offset_values(const qzk_zs_seq *seqs, uint32_t ns, uint32_t *ofv, uint32_t ofs, bool rep, int lane)
{
    uint32_t r0 = 1, r1 = 4, r2 = 8;
    for (uint32_t base = 0; base < ns; base += 64) {
        const uint32_t i = base + (uint32_t)lane, cnt = qz_uniform(ns - base < 64 ? ns - base : 64);
        uint32_t key = 0;                                           /* the offset (at most 128 KB), bit 31: literals in front */
        if (i < ns) key = seqs[i].off | (seqs[i].ll ? 1u << 31 : 0u);
        uint32_t mine = (key & 0x7fffffffu) + 3;
        if (rep) {
            for (uint32_t t = 0; t < cnt; t++) {
                const uint32_t k = qz_readlane(key, (int)t), o = k & 0x7fffffffu;
                uint32_t ov;
                if (k >> 31) {
                    if (o == r0) ov = 1;
                    else if (o == r1) { ov = 2; r1 = r0; r0 = o; }
                    else if (o == r2) { ov = 3; r2 = r1; r1 = r0; r0 = o; }
                    else { ov = o + 3; r2 = r1; r1 = r0; r0 = o; }
                } else {
                    if (o == r1) { ov = 1; r1 = r0; r0 = o; }
                    else if (o == r2) { ov = 2; r2 = r1; r1 = r0; r0 = o; }
                    else if (o == r0 - 1) { ov = 3; r2 = r1; r1 = r0; r0 = o; }        /* o >= 1: never a 0 out of rep1 == 1 */
                    else { ov = o + 3; r2 = r1; r1 = r0; r0 = o; }
                }
                if ((uint32_t)lane == t) mine = ov;
            }
        }
        if (i < ns) ofv[(uint64_t)i * ofs] = mine;
    }
    qz_wave_sync();                                                 /* the values are other lanes' stores */
}

/* the table description of norm[0..nsym) (RFC 8878, 4.1.1) into desc; returns its size.  One lane. */
QZ_DEV uint32_t qzk_zs_ncount(const int16_t *norm, uint32_t nsym, uint32_t log, uint8_t *desc)
{
    const uint32_t size = 1u << log;
    uint32_t dp = 0;
    uint64_t acc = log - 5; uint32_t nacc = 4;
    int32_t remaining = (int32_t)size + 1, threshold = (int32_t)size; uint32_t nbits = log + 1;
    uint32_t s = 0; bool prev0 = false;
    while (s < nsym && remaining > 1) {
        if (prev0) {                                                /* how many more zeros follow: 2 bits, 3 says "and then" */
            uint32_t start = s;
            while (s < nsym && !norm[s]) s++;
            while (s >= start + 3) { start += 3; acc |= 3ull << nacc; nacc += 2; }
            acc |= (uint64_t)(s - start) << nacc; nacc += 2;
        }
        int32_t c = norm[s++];
        const int32_t max = (2 * threshold - 1) - remaining;
        remaining -= c;
        c++;
        if (c >= threshold) c += max;
        acc |= (uint64_t)c << nacc; nacc += nbits;
        if (c < max) nacc--;                                        /* the short form below the threshold */
        prev0 = c == 1;
        while (remaining < threshold) { nbits--; threshold >>= 1; }
        while (nacc >= 8) { if (dp < QZK_ZS_DESCB) desc[dp] = (uint8_t)acc; dp++; acc >>= 8; nacc -= 8; }
    }
    if (nacc) { if (dp < QZK_ZS_DESCB) desc[dp] = (uint8_t)acc; dp++; }
    return dp;
}

/* table t of a chunk of ns sequences from its histogram: the mode so far (RLE, Predefined, or 2 for "FSE_Compressed if the
 * walk finds it cheaper"), and for 2 the accuracy, the counts, the description and the encoding table.  One lane per table.
 *   accuracy  log2(ns - 1) - 2 kept in 5 .. 9 (offsets: 5 .. 8), and never below log2 of the codes present, rounded up
 *   counts    count * 2^accuracy / ns rounded to nearest, at least 1 for a code that occurs; what the sum then misses goes to
 *             the most frequent code, what it has too much is taken from the then most frequent one, one at a time (the
 *             lower code among equals).  No "less than one" entries. */
QZ_DEV void qzk_zs_plan(qzk_zs_xlds *X, uint32_t t, uint32_t ns, bool fse)
{
    const uint32_t sy0 = QZK_ZS_SY0(t);
    const uint32_t *h = X->hist + sy0;
    uint32_t present = 0, top = 0;
    for (uint32_t s = 0; s < QZK_ZS_NSYM(t); s++) if (h[s]) { present++; top = s; }
    X->top[t] = top; X->dsz[t] = 0; X->log[t] = QZK_ZS_LOG(t);
    if (present == 1) { X->mode[t] = 1; return; }
    if (!fse) { X->mode[t] = 0; return; }
    X->mode[t] = 2;
    uint32_t log = qzk_zs_hb(ns - 1);                               /* two codes: ns >= 2 */
    log = log > 7 ? log - 2 : 5;
    if (log > QZK_ZS_MAXLOG(t)) log = QZK_ZS_MAXLOG(t);
    if (log < qzk_zs_hb(present - 1) + 1) log = qzk_zs_hb(present - 1) + 1;
    const uint32_t size = 1u << log, nsym = top + 1;
    int16_t *norm = X->norm + sy0;
    int32_t sum = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        int32_t n = h[s] ? (int32_t)((h[s] * size + ns / 2) / ns) : 0;
        if (h[s] && n == 0) n = 1;
        norm[s] = (int16_t)n; sum += n;
    }
    while (sum != (int32_t)size) {
        uint32_t best = 0;
        for (uint32_t s = 1; s < nsym; s++) if (norm[s] > norm[best]) best = s;
        if (sum < (int32_t)size) { norm[best] = (int16_t)(norm[best] + ((int32_t)size - sum)); sum = (int32_t)size; }
        else { norm[best]--; sum--; }                               /* the sum is above 2^accuracy >= present: the largest is above 1 */
    }
    X->log[t] = log;
    X->dsz[t] = qzk_zs_ncount(norm, nsym, log, X->desc[t]);
    qzk_zs_fse_build(norm, nsym, log, X->st + QZK_ZS_XST0(t), X->dnb + sy0, X->dfs + sy0, X->spread + QZK_ZS_XST0(t), X->cnt + sy0);
}

/* qzk_zs_sequences with `flags` (not 0): the offset values go to ofv[i * ofs] first, and each table is RLE when all codes
 * are one, else the cheaper of Predefined and FSE_Compressed by an exact count: lanes 0-2 walk the chains of the chunk's own
 * tables, lanes 3-5 those of the predefined ones, each adds up the state bits, the final state and the description; the
 * extra bits are the same either way.  On equal cost Predefined.  A code the predefined distribution does not have leaves
 * FSE_Compressed.  A trip's bits: the state bits are at most 26 a sequence where they were 17, and the extra bits of
 * lengths that add up to 128 KB at most stay under 1280 a trip, so the packer's staging area holds them. */
QZ_DEV uint32_t qzk_zs_sequences_x(qzk_zs_lds *S, qzk_zs_xlds *X, const qzk_zs_tabs *T, const qzk_zs_seq *seqs, uint32_t ns,
                                   uint32_t *ofv, uint32_t ofs, uint32_t flags, uint8_t *out, uint32_t cap, int lane)
{
    if (cap < 8) return QZK_ZS_OVER;
    if (ns == 0) { if (lane == 0) out[0] = 0; return 1; }
    uint32_t op;
    if (ns < 128) { if (lane == 0) out[0] = (uint8_t)ns; op = 1; }
    else if (ns < 0x7f00) { if (lane == 0) { out[0] = (uint8_t)((ns >> 8) + 128); out[1] = (uint8_t)ns; } op = 2; }
    else { if (lane == 0) { out[0] = 255; out[1] = (uint8_t)(ns - 0x7f00); out[2] = (uint8_t)((ns - 0x7f00) >> 8); } op = 3; }
    qzk_zs_offset_values(seqs, ns, ofv, ofs, (flags & QZK_ZS_SEQ_REP) != 0, lane);
    for (uint32_t i = (uint32_t)lane; i < 128; i += 64) X->hist[i] = 0;
    qz_lds_sync();
    for (uint32_t i = (uint32_t)lane; i < ns; i += 64) {
        const qzk_zs_codes c = qzk_zs_code_v(seqs[i].ll, seqs[i].ml, ofv[(uint64_t)i * ofs]);
        atomicAdd(&X->hist[QZK_ZS_SY0(0) + c.llc], 1u); atomicAdd(&X->hist[QZK_ZS_SY0(1) + c.ofc], 1u); atomicAdd(&X->hist[QZK_ZS_SY0(2) + c.mlc], 1u);
    }
    qz_lds_sync();
    if (lane < 3) qzk_zs_plan(X, (uint32_t)lane, ns, (flags & QZK_ZS_SEQ_FSE) != 0);
    qz_lds_sync();
    const int tl = lane < 6 ? lane % 3 : 0;
    if (X->mode[0] == 2 || X->mode[1] == 2 || X->mode[2] == 2) {    /* the walk that counts */
        const bool own = lane < 3;
        const bool walks = lane < 6 && X->mode[tl] == 2 && (own || tl != QZK_ZS_OF || X->top[QZK_ZS_OF] < QZK_ZS_OF_PREDEF);
        const uint16_t *st = own ? X->st + QZK_ZS_XST0(tl) : T->st + QZK_ZS_ST0(tl);
        const uint32_t *dnb = (own ? X->dnb : T->dnb) + QZK_ZS_SY0(tl);
        const int32_t *dfs = (own ? X->dfs : T->dfs) + QZK_ZS_SY0(tl);
        uint32_t x = 0, bits = own ? X->log[tl] + 8 * X->dsz[tl] : QZK_ZS_LOG(tl);
        for (uint32_t base = 0; base < ns; base += 64) {
            const uint32_t j = base + (uint32_t)lane, cnt = ns - base < 64 ? ns - base : 64;
            qzk_zs_codes c = { 0, 0, 0, 0, 0, 0 };
            if (j < ns) c = qzk_zs_code_v(seqs[ns - 1 - j].ll, seqs[ns - 1 - j].ml, ofv[(uint64_t)(ns - 1 - j) * ofs]);
            S->code[QZK_ZS_LL][lane] = (uint8_t)c.llc; S->code[QZK_ZS_OF][lane] = (uint8_t)c.ofc; S->code[QZK_ZS_ML][lane] = (uint8_t)c.mlc;
            qz_lds_sync();
            if (walks) {
                for (uint32_t t = 0; t < cnt; t++) {
                    const uint32_t s = S->code[tl][t];
                    if (base + t == 0) x = qzk_zs_fse_init(st, dnb, dfs, s);
                    else {
                        const uint32_t nb = (x + dnb[s]) >> 16;
                        bits += nb;
                        x = st[(int32_t)(x >> nb) + dfs[s]];
                    }
                }
            }
            qz_lds_sync();
        }
        if (lane < 6) X->cost[lane] = walks ? bits : 0xffffffffu;
        qz_lds_sync();
        if (lane < 3 && X->mode[lane] == 2 && !(X->cost[lane] < X->cost[lane + 3])) X->mode[lane] = 0;
        qz_lds_sync();
    }
    const uint32_t mll = X->mode[QZK_ZS_LL], mof = X->mode[QZK_ZS_OF], mml = X->mode[QZK_ZS_ML];
    /* the modes byte, then per table nothing, its one code, or its description: all of it or none */
    uint32_t hdr = 1;
    for (uint32_t t = 0; t < 3; t++) hdr += X->mode[t] == 1 ? 1u : X->mode[t] == 2 ? X->dsz[t] : 0u;
    if (op + hdr + 1 > cap) return QZK_ZS_OVER;
    if (lane == 0) out[op] = (uint8_t)(mll << 6 | mof << 4 | mml << 2);
    op++;
    for (uint32_t t = 0; t < 3; t++) {
        if (X->mode[t] == 1) { if (lane == 0) out[op] = (uint8_t)X->top[t]; op++; }
        else if (X->mode[t] == 2) {
            for (uint32_t i = (uint32_t)lane; i < X->dsz[t]; i += 64) out[op + i] = X->desc[t][i];
            op += X->dsz[t];
        }
    }
    /* lanes 0, 1, 2 own the LL, OF, ML chain, each in the table chosen */
    const int cl = lane < 3 ? lane : 0;
    const bool myrle = X->mode[cl] == 1, mine = X->mode[cl] == 2;
    const uint16_t *st = mine ? X->st + QZK_ZS_XST0(cl) : T->st + QZK_ZS_ST0(cl);
    const uint32_t *dnb = (mine ? X->dnb : T->dnb) + QZK_ZS_SY0(cl);
    const int32_t *dfs = (mine ? X->dfs : T->dfs) + QZK_ZS_SY0(cl);
    uint32_t x = 0;
    qzk_zs_bw w = { out + op, 0, cap - op, 0, 0, 0 };
    for (uint32_t base = 0; base < ns; base += 64) {                /* trip by trip from the last sequence back */
        const uint32_t j = base + (uint32_t)lane, cnt = ns - base < 64 ? ns - base : 64;
        qzk_zs_codes c = { 0, 0, 0, 0, 0, 0 };
        if (j < ns) c = qzk_zs_code_v(seqs[ns - 1 - j].ll, seqs[ns - 1 - j].ml, ofv[(uint64_t)(ns - 1 - j) * ofs]);
        S->code[QZK_ZS_LL][lane] = (uint8_t)c.llc; S->code[QZK_ZS_OF][lane] = (uint8_t)c.ofc; S->code[QZK_ZS_ML][lane] = (uint8_t)c.mlc;
        qz_lds_sync();
        if (lane < 3) {
            for (uint32_t t = 0; t < cnt; t++) {
                uint32_t v = 0, nb = 0;
                if (!myrle) {
                    const uint32_t s = S->code[lane][t];
                    if (base + t == 0) x = qzk_zs_fse_init(st, dnb, dfs, s);
                    else {
                        nb = (x + dnb[s]) >> 16;
                        v = x & ((1u << nb) - 1);
                        x = st[(int32_t)(x >> nb) + dfs[s]];
                    }
                }
                X->sbits[lane][t] = (uint16_t)v; S->snb[lane][t] = (uint8_t)nb;
            }
        }
        qz_lds_sync();
        uint64_t a = 0, b = 0; uint32_t na = 0, nb = 0;
        if (j < ns) {
            a = X->sbits[QZK_ZS_OF][lane]; na = S->snb[QZK_ZS_OF][lane];
            a |= (uint64_t)X->sbits[QZK_ZS_ML][lane] << na; na += S->snb[QZK_ZS_ML][lane];
            a |= (uint64_t)X->sbits[QZK_ZS_LL][lane] << na; na += S->snb[QZK_ZS_LL][lane];
            a |= (uint64_t)c.llx << na; na += QZK_ZS_LL_BITS[c.llc];
            b = c.mlx; nb = QZK_ZS_ML_BITS[c.mlc];
            b |= (uint64_t)c.ofx << nb; nb += c.ofc;
        }
        qzk_zs_pack(S, &w, a, na, b, nb, lane);
    }
    /* the final states: ML, OF, LL, each as wide as its table's accuracy, then the closing bit */
    const uint32_t xl = qz_readlane(x, 0), xo = qz_readlane(x, 1), xm = qz_readlane(x, 2);
    uint64_t a = 0; uint32_t na = 0;
    if (lane == 0) {
        const uint32_t gl = mll == 2 ? X->log[QZK_ZS_LL] : QZK_ZS_LOG(QZK_ZS_LL), go = mof == 2 ? X->log[QZK_ZS_OF] : QZK_ZS_LOG(QZK_ZS_OF),
                       gm = mml == 2 ? X->log[QZK_ZS_ML] : QZK_ZS_LOG(QZK_ZS_ML);
        if (mml != 1) { a |= (uint64_t)(xm & ((1u << gm) - 1)) << na; na += gm; }
        if (mof != 1) { a |= (uint64_t)(xo & ((1u << go) - 1)) << na; na += go; }
        if (mll != 1) { a |= (uint64_t)(xl & ((1u << gl) - 1)) << na; na += gl; }
        a |= 1ull << na; na++;
    }
    qzk_zs_pack(S, &w, a, na, 0, 0, lane);
    qzk_zs_close(&w, lane);
    return w.over ? QZK_ZS_OVER : op + w.op;
}

/* ------------------------------------------------------------------ frames */
/* records someone else made: true when every match is 3 .. 128 KB long and starts 1 .. (bytes before it) back, the literal
 * lengths stay inside the nl literals, and lengths and trailing literals add up to n */
QZ_DEV bool qzk_zs_check(const qzk_zs_seq *seqs, uint32_t ns, uint32_t nl, uint32_t n, int lane)
{
    uint32_t run = 0, lsum = 0;
    for (uint32_t base = 0; base < ns; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        qzk_zs_seq q = { 0, 0, 0 };
        bool bad = false;
        if (i < ns) {
            q = seqs[i];
            bad = q.ml < 3 || q.ml > QZK_ZS_MAXBLK || q.ll > QZK_ZS_MAXBLK || q.off == 0 || q.off > QZK_ZS_MAXBLK;
            if (bad) { q.ll = 0; q.ml = 0; }
        }
        const uint32_t incl = qz_wave_incl_scan(q.ll + q.ml), lincl = qz_wave_incl_scan(q.ll);
        if (i < ns && q.off > run + incl - q.ml) bad = true;
        run += qz_readlane(incl, 63); lsum += qz_readlane(lincl, 63);
        if (qz_ballot(bad) || run > n || lsum > nl) return false;
    }
    return run + (nl - lsum) == n;
}

/* the content of checked records, for the Raw block of a frame that has no source to copy */
QZ_DEV void qzk_zs_rebuild(uint8_t *dst, const qzk_zs_seq *seqs, uint32_t ns, const uint8_t *lits, uint32_t nl, int lane)
{
    uint32_t p = 0, lp = 0;
    for (uint32_t s = 0; s < ns; s++) {
        const qzk_zs_seq q = seqs[s];
        qzk_wave_copy(dst + p, lits + lp, q.ll, lane);
        p += q.ll; lp += q.ll;
        qz_wave_sync();
        for (uint32_t i = (uint32_t)lane; i < q.ml; i += 64) dst[p + i] = dst[p - q.off + i % q.off];
        p += q.ml;
        qz_wave_sync();
    }
    qzk_wave_copy(dst + p, lits + lp, nl - lp, lane);
}

/* one frame of n >= 1 bytes at out (QZK_ZS_BOUND(n) + QZK_ZS_SLACK bytes are there); src: the content, NULL when the records
 * are all there is.  Returns the frame's size, at most QZK_ZS_BOUND(n). */
/* SEQ: the sequences section is qzk_zs_sequences_x's under `flags` (X, ofv and ofs are its arguments), else qzk_zs_sequences' */
template <bool SEQ>
QZ_DEV uint32_t qzk_zs_frame(qzk_zs_lds *S, qzk_zs_xlds *X, const qzk_zs_tabs *T, const uint8_t *src, uint32_t n, const qzk_zs_seq *seqs,
                             uint32_t ns, uint32_t *ofv, uint32_t ofs, uint32_t flags, const uint8_t *lits, uint32_t nl, uint8_t *out, int lane)
{
    const uint32_t fb = n < 256 ? 1u : n < 65792 ? 2u : 4u;
    if (lane == 0) {
        out[0] = 0x28; out[1] = 0xb5; out[2] = 0x2f; out[3] = 0xfd;
        out[4] = (uint8_t)(0x20 | (fb == 1 ? 0u : fb == 2 ? 1u : 2u) << 6);
        const uint32_t v = fb == 2 ? n - 256 : n;
        for (uint32_t i = 0; i < fb; i++) out[5 + i] = (uint8_t)(v >> (8 * i));
    }
    const uint32_t hp = 5 + fb;
    uint8_t *body = out + hp + 3;
    uint32_t bsz = QZK_ZS_OVER;
    const uint32_t lsz = qzk_zs_literals(S, lits, nl, body, lane);
    if (lsz < n) {
        const uint32_t ssz = SEQ ? qzk_zs_sequences_x(S, X, T, seqs, ns, ofv, ofs, flags, body + lsz, n - lsz, lane)
                                 : qzk_zs_sequences(S, T, seqs, ns, body + lsz, n - lsz, lane);
        if (ssz != QZK_ZS_OVER && lsz + ssz < n) bsz = lsz + ssz;
    }
    uint32_t bh;
    if (bsz != QZK_ZS_OVER) bh = 1u | 2u << 1 | bsz << 3;
    else {
        qz_wave_sync();
        if (src) qzk_wave_copy(body, src, n, lane);
        else qzk_zs_rebuild(body, seqs, ns, lits, nl, lane);
        bsz = n; bh = 1u | n << 3;
    }
    if (lane == 0) { out[hp] = (uint8_t)bh; out[hp + 1] = (uint8_t)(bh >> 8); out[hp + 2] = (uint8_t)(bh >> 16); }
    return hp + 3 + bsz;
}

/* what a wave needs beside LDS for a chunk of up to block_sz bytes: the literals, then the records (a record covers at least
 * three bytes) */
#define QZK_ZS_LITB(block_sz) (((block_sz) + 15u) & ~15u)
#define QZK_ZS_WAVEB(block_sz) (QZK_ZS_LITB(block_sz) + ((((block_sz) / 3u + 1u) * 12u + 15u) & ~15u))

/* Kz: persistent single-wave workgroups pull chunk numbers (as qzk_lz4s_pull_kernel); chunk b of the launch goes to slot b as
 * one frame, out_len[b] = its size.  scratch: QZK_ZS_WAVEB(block_sz) bytes per workgroup of the launch.  With SEQ the
 * offset values overwrite the records' offsets in the wave's scratch, and the chunk's tables lie behind the stage's LDS. */
template <bool SEQ>
QZ_DEV void qzk_zstd_pull(uint32_t *table, const qzk_zs_tabs *T, const uint8_t *src, uint64_t src_len, uint32_t block_sz, uint32_t nblocks,
                          uint8_t *slots, uint32_t stride, uint32_t *out_len, uint32_t mm, uint32_t *counter, uint8_t *scratch, uint32_t flags)
{
    const int lane = qz_lane();
    uint8_t *lits = scratch + (uint64_t)blockIdx.x * QZK_ZS_WAVEB(block_sz);
    qzk_zs_seq *seqs = (qzk_zs_seq *)(lits + QZK_ZS_LITB(block_sz));
    for (;;) {
        uint32_t b = atomicAdd(counter, lane == 0 ? 1u : 0u);
        b = qz_readfirstlane(b);
        if (b >= nblocks) break;
        const uint64_t off = (uint64_t)b * block_sz;
        const uint32_t n = (uint32_t)((src_len - off) < block_sz ? (src_len - off) : block_sz);
        qzk_zs_rec e = { seqs, lits, 0, 0 };
        qzk_l4s_parse(src + off, n, e, mm, table, lane);
        qz_wave_sync();                                             /* the records and literals are other lanes' stores */
        const uint32_t c = qzk_zs_frame<SEQ>((qzk_zs_lds *)table, (qzk_zs_xlds *)((uint8_t *)table + QZK_ZS_XOFF), T, src + off, n, seqs, e.ns,
                                             &seqs[0].off, 3, flags, lits, e.nl, slots + (uint64_t)b * stride, lane);
        out_len[b] = c;                 /* wave-uniform: every lane stores the same word */
        qz_wave_sync();
    }
}
QZ_KERNEL_MAX(64) qzk_zstd_pull_kernel(const uint8_t *src, uint64_t src_len, uint32_t block_sz, uint32_t nblocks, uint8_t *slots,
                                       uint32_t stride, uint32_t *out_len, uint32_t mm, uint32_t *counter, uint8_t *scratch)
{
    QZ_LDS uint32_t table[QZK_L4S_HSIZE];
    QZ_LDS qzk_zs_tabs T;
    qzk_zs_tabs_init(&T, qz_lane());
    qzk_zstd_pull<false>(table, &T, src, src_len, block_sz, nblocks, slots, stride, out_len, mm, counter, scratch, 0);
}
/* ... with seq_flags (not 0): a kernel of its own, so that the one above stays what it was */
QZ_KERNEL_MAX(64) qzk_zstd_pull_seq_kernel(const uint8_t *src, uint64_t src_len, uint32_t block_sz, uint32_t nblocks, uint8_t *slots,
                                           uint32_t stride, uint32_t *out_len, uint32_t mm, uint32_t *counter, uint8_t *scratch,
                                           uint32_t seq_flags)
{
    QZ_LDS uint32_t table[QZK_L4S_HSIZE];
    QZ_LDS qzk_zs_tabs T;
    qzk_zs_tabs_init(&T, qz_lane());
    qzk_zstd_pull<true>(table, &T, src, src_len, block_sz, nblocks, slots, stride, out_len, mm, counter, scratch, seq_flags);
}

/* the entropy stage alone, a wave per frame of the caller's records: out_len[b] = the frame's size, or 0 and *bad set when
 * the records are not a frame's (qzk_zs_check).  With SEQ the offset values go to ofv + workgroup * ofv_words: the caller's
 * records are not written. */
template <bool SEQ>
QZ_DEV void qzk_zstd_encode(qzk_zs_lds *S, qzk_zs_xlds *X, const qzk_zs_tabs *T, const uint8_t *lits, const qzk_zs_seq *seqs,
                            const qzk_zs_fdesc *desc, uint32_t nframes, uint8_t *slots, uint32_t stride, uint32_t *out_len, uint32_t *bad,
                            uint32_t *counter, uint32_t *ofv, uint32_t ofv_words, uint32_t flags)
{
    const int lane = qz_lane();
    uint32_t *myofv = SEQ ? ofv + (uint64_t)blockIdx.x * ofv_words : NULL;
    for (;;) {
        uint32_t b = atomicAdd(counter, lane == 0 ? 1u : 0u);
        b = qz_readfirstlane(b);
        if (b >= nframes) break;
        const qzk_zs_fdesc d = desc[b];
        uint32_t c = 0;
        if (qzk_zs_check(seqs + d.seq0, d.nseq, d.nlit, d.content, lane) && (!SEQ || d.nseq <= ofv_words))
            c = qzk_zs_frame<SEQ>(S, X, T, NULL, d.content, seqs + d.seq0, d.nseq, myofv, 1, flags, lits + d.lit0, d.nlit,
                                  slots + (uint64_t)b * stride, lane);
        else if (lane == 0) atomicOr(bad, 1u);
        out_len[b] = c;
        qz_wave_sync();
    }
}
QZ_KERNEL_MAX(64) qzk_zstd_encode_kernel(const uint8_t *lits, const qzk_zs_seq *seqs, const qzk_zs_fdesc *desc, uint32_t nframes,
                                         uint8_t *slots, uint32_t stride, uint32_t *out_len, uint32_t *bad, uint32_t *counter)
{
    QZ_LDS qzk_zs_lds S;
    QZ_LDS qzk_zs_tabs T;
    qzk_zs_tabs_init(&T, qz_lane());
    qzk_zstd_encode<false>(&S, NULL, &T, lits, seqs, desc, nframes, slots, stride, out_len, bad, counter, NULL, 0, 0);
}
QZ_KERNEL_MAX(64) qzk_zstd_encode_seq_kernel(const uint8_t *lits, const qzk_zs_seq *seqs, const qzk_zs_fdesc *desc, uint32_t nframes,
                                             uint8_t *slots, uint32_t stride, uint32_t *out_len, uint32_t *bad, uint32_t *counter,
                                             uint32_t *ofv, uint32_t ofv_words, uint32_t seq_flags)
{
    QZ_LDS qzk_zs_lds S;
    QZ_LDS qzk_zs_xlds X;
    QZ_LDS qzk_zs_tabs T;
    qzk_zs_tabs_init(&T, qz_lane());
    qzk_zstd_encode<true>(&S, &X, &T, lits, seqs, desc, nframes, slots, stride, out_len, bad, counter, ofv, ofv_words, seq_flags);
}

#endif
