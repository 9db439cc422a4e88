/*
 * qzk_zstdd_blocks.h — the block route of the zstd decoder: the bit streams of a multi-block frame (what zstd, ZSTD_compress
 * and ZSTD_compressStream write: one frame, thousands of 128 KB blocks) read a block per lane group instead of one after
 * the other on the frame's lanes (stage E of qzk_zstdd.h).  Five launches on one stream, no kernel waits on another wave:
 *
 *   Plan    (qzk_zstdd_bplan_kernel)    a wave per routed frame, its lane 0 serial over the frame's blocks: the frame header,
 *           then per block the 3-byte header, the literals section's header, the sequence count and the mode byte - nothing
 *           that needs a bit stream - into one descriptor per block: where the block lies, where its literals and its
 *           records go (prefixes of the regenerated sizes and of nseq + 1), which earlier block's Huffman tree it uses and
 *           which earlier block last set each of LL / OF / ML with a mode other than Repeat.  Refusals a header shows are
 *           recorded with the block.  A block count other than the caller's is QZK_ZD_EHINT for the frame.
 *   Entropy (qzk_zstdd_bentropy_kernel) QZK_ZD_L lanes per BLOCK, QZK_ZD_G blocks a wave, the lane roles and the LDS struct
 *           of stage E.  Inherited tables are rebuilt from the input: the leader parses the defining blocks again
 *           (qzk_zd_block, in ascending order, so a later definition overrides an earlier one as it does in the frame), puts
 *           back the predefined distribution where that is what the block inherits, then parses the block itself.  The sequence lane starts from a symbolic history: a slot is a distance, or "incoming slot k
 *           minus d".  A record whose distance came from the incoming history carries k + 1 in bits 30-31 of its match
 *           length (lengths need 18 bits; the distance keeps its 32) and d as its distance.  Per block: the bytes produced,
 *           the outgoing history in symbolic form, the records written and the first refusal with its record's index.  The
 *           checks that need no output position are made here.
 *   Scan    (qzk_zstdd_bscan_kernel)    per frame, serial over descriptors: each block's output start and its concrete
 *           incoming history, from 1 / 4 / 8.
 *   Fix     (qzk_zstdd_bfix_kernel)     a wave per block: tagged records become plain distances; the position-dependent checks
 *           (distance 0, distance > produced + ll, QZK_ZD_EOUT, the block maximum, content overrun) in sequence order over a
 *           wave prefix sum of ll + ml; the earliest failing record is kept.
 *   Finish  (qzk_zstdd_bfinish_kernel)  per frame: the status is that of the earliest failure in stream order - block index,
 *           then record index, a block's header refusals before its records, and at one record what the bit stream shows
 *           before what the position shows, which is the order stage E meets them in.  Then the end-of-frame checks and the
 *           frame's qzk_zdres exactly as stage E writes it.
 *
 * Stage X and the checksum kernel then run unchanged.  Every block owns exactly nseq + 1 records of the frame's region: a
 * block without trailing literals (and an empty Raw or RLE block) gets the record {0, 0, 0}, which is a no-op in the copy
 * engine (a lane with no literals and no match, as its idle lanes are); Fix does not compact.
 * The record region of a block is cut at the frame's rec_cap: a frame whose blocks announce more records than rec_cap holds
 * produces more than out_cap before the cut (qzd_zd_caps), so an earlier record already answers QZK_ZD_EOUT or worse.
 */
#ifndef QZK_ZSTDD_BLOCKS_H
#define QZK_ZSTDD_BLOCKS_H
#include "qzk_zstdd.h"

#define QZK_ZD_EHINT (-6)           /* the frame's block count is not the caller's */
#define QZK_ZDB_NONE (-1)           /* nothing to inherit yet */
#define QZK_ZDB_UNUSED (-3)         /* the block inherits none */
#define QZK_ZDB_PREDEF (-2)         /* the predefined distribution */
#define QZK_ZDB_MLMASK 0x3fffffffu

typedef struct {
    /* Plan */
    uint32_t in_off, bsz, flags;                    /* the block header's place in the frame; Block_Size; type | last << 2 */
    int32_t herr;                                   /* what its headers refuse it with */
    uint32_t lit_regen, lit_pre, nseq, rec_pre;
    int32_t huf_blk, tab_blk[3];
    /* Entropy */
    uint32_t bprod, nrec;
    int32_t err; uint32_t err_rec;
    uint32_t rep_tag[3], rep_val[3];                /* outgoing history: tag 0 a distance, tag k + 1 incoming slot k minus val */
    /* Scan */
    uint32_t rep_in[3], pad;
    uint64_t out_start;
    /* Fix */
    int32_t ferr; uint32_t ferr_rec;
} qzk_zdb_desc;

/* a routed frame: seg, hint, first_blk by the host; the rest by Plan and Scan */
typedef struct {
    uint32_t seg, hint, first_blk;                  /* its segment of the round; the caller's block count; its first descriptor */
    int32_t status; uint32_t decided;               /* decided: the frame's answer is status, no block of it runs */
    uint32_t nblk, complete, pos_end;               /* descriptors written; the walk reached the last block; the input behind it */
    uint32_t bmax, content, has_content, has_cksum;
    uint64_t produced;
} qzk_zdb_frame;

/* the literals section's header and the sequences section's count and mode byte of a Compressed block b[0 .. bsz): a subset of
 * qzk_zd_block's checks, all of them QZK_ZD_EDATA there too */
QZ_DEV int qzk_zdb_sections(const uint8_t *b, uint32_t bsz, uint32_t *lt, uint32_t *regen, uint32_t *nseq_out, uint32_t *modes_out)
{
    if (bsz < 1) return QZK_ZD_EDATA;
    const uint32_t t = b[0] & 3, fmt = (b[0] >> 2) & 3;
    uint32_t lend, n;
    if (t < 2) {
        const uint32_t hs = !(fmt & 1) ? 1u : fmt == 1 ? 2u : 3u;
        if (bsz < hs) return QZK_ZD_EDATA;
        uint32_t v = b[0];
        if (hs > 1) v |= (uint32_t)b[1] << 8;
        if (hs > 2) v |= (uint32_t)b[2] << 16;
        n = v >> (hs == 1 ? 3 : 4);
        if (n > QZK_ZD_MAXBLK) return QZK_ZD_EDATA;
        if (t == 0) { if (bsz - hs < n) return QZK_ZD_EDATA; lend = hs + n; }
        else { if (bsz - hs < 1) return QZK_ZD_EDATA; lend = hs + 1; }
    } else {
        const uint32_t hs = fmt < 2 ? 3u : fmt == 2 ? 4u : 5u, bits = fmt < 2 ? 10u : fmt == 2 ? 14u : 18u;
        if (bsz < hs) return QZK_ZD_EDATA;
        uint64_t v = 0;
        for (uint32_t i = 0; i < hs; i++) v |= (uint64_t)b[i] << (8 * i);
        v >>= 4;
        n = (uint32_t)(v & ((1u << bits) - 1));
        const uint32_t csz = (uint32_t)(v >> bits);
        if (n > QZK_ZD_MAXBLK) return QZK_ZD_EDATA;
        if (bsz - hs < csz) return QZK_ZD_EDATA;
        lend = hs + csz;
    }
    const uint8_t *q = b + lend;
    const uint32_t qlen = bsz - lend;
    if (qlen < 1) return QZK_ZD_EDATA;
    uint32_t nseq, qp;
    if (q[0] < 128) { nseq = q[0]; qp = 1; }
    else if (q[0] < 255) { if (qlen < 2) return QZK_ZD_EDATA; nseq = ((uint32_t)(q[0] - 128) << 8) + q[1]; qp = 2; }
    else { if (qlen < 3) return QZK_ZD_EDATA; nseq = q[1] + ((uint32_t)q[2] << 8) + 0x7f00; qp = 3; }
    uint32_t modes = 0;
    if (nseq) {
        if (qp >= qlen) return QZK_ZD_EDATA;
        modes = q[qp];
        if (modes & 3) return QZK_ZD_EDATA;
    }
    *lt = t; *regen = n; *nseq_out = nseq; *modes_out = modes;
    return 0;
}

/* Plan.  grid: one single-wave workgroup per routed frame.  desc NULL: the walk alone, counts[f] <- the frame's blocks (0
 * where the walk does not reach the frame's end) - qzd_zstd_count_blocks */
QZ_KERNEL_MAX(64) qzk_zstdd_bplan_kernel(const uint8_t *comp, const qzk_zdseg *segs, const qzk_zdplan *plan, qzk_zdb_frame *frames,
                                         uint32_t nframes, qzk_zdb_desc *desc, uint32_t *counts)
{
    const uint32_t f = blockIdx.x;
    if (f >= nframes || qz_lane() != 0) return;
    qzk_zd_frame Fs;                                                /* (qzk_zd_frame_header touches six words of it: they stay in registers) */
    qzk_zd_frame *const F = &Fs;
    qzk_zdb_frame fr = frames[f];
    const qzk_zdseg sg = segs[fr.seg];
    const uint8_t *const in = comp + sg.in_off;
    uint32_t lit_cap = 0xffffffffu;
    if (desc) lit_cap = plan[fr.seg].lit_cap;
    fr.status = 0; fr.decided = 0; fr.nblk = 0; fr.complete = 0; fr.pos_end = 0; fr.produced = 0;
    F->pos = 0; F->bmax = 0; F->content = 0; F->has_content = 0; F->has_cksum = 0;
    uint32_t skip = 0;
    const int he = qzk_zd_frame_header(F, in, sg.in_len, desc ? sg.out_cap : 0xffffffffu, &skip);
    fr.bmax = F->bmax; fr.content = F->content; fr.has_content = F->has_content; fr.has_cksum = F->has_cksum;
    if (he) { fr.status = he; fr.decided = 1; }
    else if (skip) { fr.complete = 1; fr.pos_end = F->pos; }
    else {
        qzk_zdb_desc *const D = desc ? desc + fr.first_blk : desc;
        uint32_t pos = F->pos, b = 0, lit_pre = 0;
        uint64_t rec_pre = 0;
        int32_t cur_huf = QZK_ZDB_NONE, cur_tab[3] = { QZK_ZDB_NONE, QZK_ZDB_NONE, QZK_ZDB_NONE };
        for (;;) {
            if (b >= fr.hint) { fr.status = QZK_ZD_EHINT; fr.decided = 1; break; }          /* more blocks than descriptors */
            qzk_zdb_desc d;
            d.in_off = pos; d.bsz = 0; d.flags = 3; d.herr = 0; d.lit_regen = 0; d.lit_pre = lit_pre; d.nseq = 0;
            d.rec_pre = (uint32_t)rec_pre; d.huf_blk = QZK_ZDB_UNUSED; d.tab_blk[0] = d.tab_blk[1] = d.tab_blk[2] = QZK_ZDB_UNUSED;
            d.bprod = 0; d.nrec = 0; d.err = 0; d.err_rec = 0;
            for (uint32_t k = 0; k < 3; k++) { d.rep_tag[k] = k + 1; d.rep_val[k] = 0; d.rep_in[k] = 0; }
            d.pad = 0; d.out_start = 0; d.ferr = 0; d.ferr_rec = 0;
            bool stop = false;
            uint32_t last = 0;
            if (sg.in_len - pos < 3) { d.herr = QZK_ZD_ETRUNC; stop = true; }
            else {
                const uint32_t bh = in[pos] | (uint32_t)in[pos + 1] << 8 | (uint32_t)in[pos + 2] << 16;
                const uint32_t type = (bh >> 1) & 3, bsz = bh >> 3;
                last = bh & 1;
                d.bsz = bsz; d.flags = type | last << 2;
                const uint32_t body = pos + 3, need = type == 1 ? 1u : bsz;
                if (type == 3 || bsz > fr.bmax) { d.herr = QZK_ZD_EDATA; stop = true; }
                else if (sg.in_len - body < need) { d.herr = QZK_ZD_ETRUNC; stop = true; }
                else if (type != 2) {
                    const uint32_t regen = type == 0 ? bsz : bsz ? 1u : 0u;
                    /* (behind literals that fill lit_cap = out_cap the block's bytes are beyond out_cap) */
                    if (regen > lit_cap - lit_pre) d.herr = QZK_ZD_EOUT; else d.lit_regen = regen;
                    pos = body + need;
                } else {
                    uint32_t t = 0, regen = 0, nseq = 0, modes = 0;
                    if (qzk_zdb_sections(in + body, bsz, &t, &regen, &nseq, &modes)) d.herr = QZK_ZD_EDATA;
                    else if (regen > lit_cap - lit_pre) d.herr = QZK_ZD_EDATA;
                    else {
                        d.lit_regen = regen; d.nseq = nseq;
                        if (t == 3) d.huf_blk = cur_huf;
                        if (t == 2) cur_huf = (int32_t)b;
                        if (nseq) for (uint32_t k = 0; k < 3; k++) {
                            const uint32_t mode = (modes >> (6 - 2 * k)) & 3;
                            if (mode == 3) d.tab_blk[k] = cur_tab[k];
                            else cur_tab[k] = mode == 0 ? QZK_ZDB_PREDEF : (int32_t)b;
                        }
                    }
                    pos = body + bsz;
                }
            }
            if (D) D[b] = d;
            lit_pre += d.lit_regen;
            rec_pre += (uint64_t)d.nseq + 1;
            if (rec_pre > 0xfffffff0ull) rec_pre = 0xfffffff0ull;
            b++;
            if (stop) break;
            if (last) { fr.complete = 1; break; }
        }
        fr.nblk = b; fr.pos_end = pos;
    }
    if (!fr.decided && fr.complete && fr.nblk != fr.hint && desc) { fr.status = QZK_ZD_EHINT; fr.decided = 1; }
    if (desc) frames[f] = fr;
    /* (the host's walk, qzd_zd_frame_walk, wants the checksum's four bytes too) */
    if (counts) counts[f] = fr.complete && !fr.decided && !(fr.has_cksum && sg.in_len - fr.pos_end < 4) ? fr.nblk : 0;
}

/* the routed frame of the global block index gb: the last one whose first_blk <= gb */
QZ_DEV uint32_t qzk_zdb_frame_of(const qzk_zdb_frame *frames, uint32_t nframes, uint32_t gb)
{
    uint32_t lo = 0, hi = nframes;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (frames[mid].first_blk <= gb) lo = mid; else hi = mid; }
    return lo;
}

/* a group's passes: the blocks its leader parses, the last one its own; bad: an inherited table could not be rebuilt */
typedef struct { uint32_t final, npass, pi, bad, pass[5]; } qzk_zdb_ctl;

/* Entropy.  grid: ceil(nblocks / QZK_ZD_G) single-wave workgroups, nblocks = the sum of the frames' hints */
QZ_KERNEL_MAX(64) qzk_zstdd_bentropy_kernel(const uint8_t *comp, const qzk_zdseg *segs, const qzk_zdplan *plan, const qzk_zdb_frame *frames,
                                            uint32_t nframes, uint32_t nblocks, qzk_zdb_desc *desc, uint8_t *scratch)
{
    QZ_LDS qzk_zd_frame groups[QZK_ZD_G];
    QZ_LDS qzk_zdb_ctl ctl[QZK_ZD_G];
    const uint32_t lane = (uint32_t)qz_lane(), g = lane / QZK_ZD_L, r = lane % QZK_ZD_L;
    const uint32_t gb = blockIdx.x * QZK_ZD_G + g;
    qzk_zd_frame *const F = &groups[g];
    qzk_zdb_ctl *const C = &ctl[g];
    bool valid = gb < nblocks;
    qzk_zdseg sg; sg.in_off = 0; sg.out_off = 0; sg.in_len = 0; sg.out_cap = 0;
    qzk_zdplan pl; pl.lit_off = 0; pl.rec_off = 0; pl.lit_cap = 0; pl.rec_cap = 0;
    uint32_t b = 0, first_blk = 0, bmax = 0;
    if (valid) {
        const qzk_zdb_frame *fr = frames + qzk_zdb_frame_of(frames, nframes, gb);
        first_blk = fr->first_blk; b = gb - first_blk; bmax = fr->bmax;
        valid = !fr->decided && b < fr->nblk;
        if (valid) { sg = segs[fr->seg]; pl = plan[fr->seg]; }
    }
    qzk_zdb_desc *const D = desc + first_blk;
    qzk_zdb_desc *const me = D + b;
    if (valid) valid = me->herr == 0;
    const uint8_t *const in = comp + sg.in_off;
    uint8_t *const lit = scratch + pl.lit_off;
    uint32_t rec_pre = 0, rcap = 0;
    if (valid) {
        rec_pre = me->rec_pre;
        if (rec_pre < pl.rec_cap) { rcap = pl.rec_cap - rec_pre; if (rcap > me->nseq + 1) rcap = me->nseq + 1; } else rec_pre = 0;
    }
    uint32_t *const rec = (uint32_t *)(scratch + pl.rec_off) + 3 * (size_t)rec_pre;
    /* the leader's passes: the blocks that define what this one inherits, ascending, then the block itself */
    if (r == 0) {
        F->pos = 0; F->bmax = bmax; F->content = 0; F->produced = 0; F->nlit = 0; F->nrec = 0; F->has_content = 0; F->has_cksum = 0;
        F->have_huf = 0; F->have_seq = 0; F->hlog = 0; F->nsym = 0; F->done = 0; F->err = 0;
        F->tkind[0] = F->tkind[1] = F->tkind[2] = 0;
        F->btype = 3; F->huf_new = 0; F->build[0] = F->build[1] = F->build[2] = 0; F->lit_kind = 0; F->nstreams = 0; F->nseq = 0;
        F->lit_regen = 0; F->q_len = 0;
        for (uint32_t i = 0; i < 8; i++) F->serr[i] = 0;
        C->final = valid ? 0u : 1u; C->npass = 0; C->pi = 0; C->bad = 0;
        if (valid) {
            int32_t want[4] = { me->huf_blk, me->tab_blk[0], me->tab_blk[1], me->tab_blk[2] };
            for (;;) {                                              /* the smallest one above the last taken */
                int32_t best = -1;
                for (uint32_t i = 0; i < 4; i++)
                    if (want[i] >= 0 && (uint32_t)want[i] < b && (C->npass == 0 || (uint32_t)want[i] > C->pass[C->npass - 1]) && (best < 0 || want[i] < best))
                        best = want[i];
                if (best < 0) break;
                C->pass[C->npass++] = (uint32_t)best;
            }
            C->pass[C->npass++] = b;
        }
    }
    qz_wave_sync();
    while (qz_ballot(valid && !C->final) != 0) {
        const bool active = valid && !C->final;
        qz_wave_sync();                                             /* everyone has read `final` before the leader may change it */
        /* ---- 1: the leader reads a block's headers: a defining block's for its tables, or the block's own ---- */
        if (active && r == 0) {
            const uint32_t d = C->pass[C->pi++];
            if (F->serr[5] || F->serr[6] || F->serr[7]) C->bad = 1;
            for (uint32_t i = 0; i < 8; i++) F->serr[i] = 0;
            if (C->pi < C->npass) {
                /* what the defining block itself inherits is no concern here; a block that does not parse refuses the frame at
                 * its own index, before this one */
                F->pos = D[d].in_off; F->have_huf = 1; F->have_seq = 1; F->nlit = 0; F->nrec = 0; F->produced = 0;
                const int e = (D[d].flags & 3) == 2 ? qzk_zd_block(F, in, sg.in_len, 0xffffffffu, lit, 0xffffffffu, rec, 0) : QZK_ZD_EDATA;
                if (e) { F->btype = 3; F->huf_new = 0; C->bad = 1; }
                F->err = 0;
            } else {
                F->pos = me->in_off; F->nlit = me->lit_pre; F->nrec = 0; F->produced = 0;
                F->have_huf = me->huf_blk >= 0;
                F->have_seq = me->tab_blk[0] != QZK_ZDB_NONE && me->tab_blk[1] != QZK_ZDB_NONE && me->tab_blk[2] != QZK_ZDB_NONE;
                F->err = C->bad ? QZK_ZD_EDATA : qzk_zd_block(F, in, sg.in_len, 0xffffffffu, lit, pl.lit_cap, rec, rcap);
                /* An inherited predefined table is put back only now, for the table lanes to build with the block's own: a
                 * pass over a defining block rebuilds all of that block's tables, also one that a later block - no definer of
                 * anything this block inherits, so it has no pass - set back to the predefined distribution.  The block's own
                 * mode for such a table is Repeat: its parse has left the table and its counts alone. */
                if (!F->err && F->btype == 2) for (uint32_t k = 0; k < 3; k++) if (me->tab_blk[k] == QZK_ZDB_PREDEF && F->tkind[k] != 1) {
                    const int16_t *src = k == 0 ? qzk_zd_ll_norm : k == 1 ? qzk_zd_of_norm : qzk_zd_ml_norm;
                    const uint32_t ns = k == 0 ? 36u : k == 1 ? 29u : 53u;
                    for (uint32_t i = 0; i < ns; i++) F->norm[k][i] = src[i];
                    F->nsymb[k] = ns; F->tlog[k] = k == 1 ? 5u : 6u; F->build[k] = 1; F->tkind[k] = 1;
                }
                C->final = 1;
            }
        }
        qz_wave_sync();
        const bool work = active && F->err == 0;
        const bool own = work && C->final;
        /* ---- 2: the tables ---- */
        if (work && F->btype == 2) {
            if (r >= 5 && r <= 7 && F->build[r - 5]) {
                const uint32_t k = r - 5;
                F->serr[r] = qzk_zd_fse_build(F->norm[k], F->nsymb[k], F->tlog[k], k == 0 ? F->ll : k == 1 ? F->of : F->ml, F->nxt[k]);
            }
            if (F->huf_new) qzk_zd_huf_fill(F, r);
        }
        qz_wave_sync();
        /* ---- 3: the block's own streams, one lane each; Raw and RLE bytes by all the group's lanes ---- */
        {
            const bool tables_ok = own && F->serr[5] == 0 && F->serr[6] == 0 && F->serr[7] == 0;
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
            /* the sequence lane: the history is symbolic (tag 0: a distance; tag k + 1: incoming slot k minus val) */
            qzk_zd_bits qb; qb.base = in; qb.ptr = 0; qb.used = 64; qb.c = 0;
            uint32_t qleft = 0, sl = 0, so = 0, sm = 0, lit_used = 0, nrec = 0, bprod = 0, at = 0;
            uint32_t t0 = 1, v0 = 0, t1 = 2, v1 = 0, t2 = 3, v2 = 0;
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
                        uint32_t dt, dv;
                        if (ov > 3) { dt = 0; dv = ov - 3; t2 = t1; v2 = v1; t1 = t0; v1 = v0; t0 = dt; v0 = dv; }
                        else {
                            const uint32_t idx = ov - 1 + (ll == 0 ? 1u : 0u);
                            if (idx == 0) { dt = t0; dv = v0; }
                            else {
                                if (idx == 1) { dt = t1; dv = v1; }
                                else if (idx == 2) { dt = t2; dv = v2; }
                                else { dt = t0; dv = t0 ? v0 + 1 : v0 - 1; }
                                if (idx != 1) { t2 = t1; v2 = v1; }
                                t1 = t0; v1 = v0; t0 = dt; v0 = dv;
                            }
                        }
                        lit_used += ll;
                        if (!qerr) {
                            if ((dt == 0 && dv == 0) || lit_used > lit_regen) qerr = QZK_ZD_EDATA;
                            else qerr = qzk_zd_record(rec, rcap, &nrec, ll, ml | dt << 30, dv);
                        }
                        if (bprod < 0x40000000u) bprod += ll + ml;  /* (beyond any block maximum it only has to stay beyond) */
                        qleft--;
                        if (qerr) qleft = 0;
                        else {
                            at++;
                            if (qleft) {
                                sl = (el >> 16) + qzk_zd_bits_read(&qb, (el >> 8) & 0xff, &qerr);
                                sm = (em >> 16) + qzk_zd_bits_read(&qb, (em >> 8) & 0xff, &qerr);
                                so = (eo >> 16) + qzk_zd_bits_read(&qb, (eo >> 8) & 0xff, &qerr);
                                if (qerr) qleft = 0;
                            }
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
                if (!qerr) {
                    const uint32_t rest = lit_regen - lit_used;     /* the block's last record, a no-op where nothing trails */
                    qerr = qzk_zd_record(rec, rcap, &nrec, rest, 0, 0);
                    bprod += rest;
                }
                F->serr[4] = qerr; F->produced = bprod; F->nrec = nrec;
                F->rank[0] = t0; F->rank[1] = t1; F->rank[2] = t2; F->rank[3] = v0; F->rank[4] = v1; F->rank[5] = v2; F->rank[6] = at;
            }
        }
        qz_wave_sync();
        /* ---- 4: the leader leaves the block's answers in its descriptor ---- */
        if (active && C->final && r == 0) {
            int e = F->err;
            for (uint32_t i = 0; i < 8 && !e; i++) if (i != 4) e = F->serr[i];
            if (e) { me->err = e; me->err_rec = 0; me->nrec = 0; me->bprod = 0; }      /* before any record of the block */
            else if (F->btype == 2) {
                me->err = F->serr[4]; me->err_rec = F->rank[6]; me->nrec = F->nrec; me->bprod = F->produced;
                for (uint32_t k = 0; k < 3; k++) { me->rep_tag[k] = F->rank[k]; me->rep_val[k] = F->rank[3 + k]; }
            } else {
                /* Raw and RLE: qzk_zd_block wrote the record; an empty block's is the no-op */
                if (F->nrec == 0) e = qzk_zd_record(rec, rcap, &F->nrec, 0, 0, 0);
                me->err = e; me->err_rec = 0; me->nrec = e ? 0 : 1; me->bprod = me->bsz;
            }
        }
        qz_wave_sync();
    }
}

/* Scan.  grid: one single-wave workgroup per routed frame */
QZ_KERNEL_MAX(64) qzk_zstdd_bscan_kernel(qzk_zdb_frame *frames, uint32_t nframes, qzk_zdb_desc *desc)
{
    const uint32_t f = blockIdx.x;
    if (f >= nframes || qz_lane() != 0) return;
    const qzk_zdb_frame fr = frames[f];
    if (fr.decided) return;
    qzk_zdb_desc *const D = desc + fr.first_blk;
    uint64_t start = 0;
    uint32_t rep[3] = { 1, 4, 8 };
    for (uint32_t b = 0; b < fr.nblk; b++) {
        qzk_zdb_desc *d = D + b;
        d->out_start = start;
        uint32_t nx[3];
        for (uint32_t k = 0; k < 3; k++) {
            d->rep_in[k] = rep[k];
            const uint32_t t = d->rep_tag[k], v = d->rep_val[k];
            nx[k] = t == 0 ? v : (t == 1 ? rep[0] : t == 2 ? rep[1] : rep[2]) - v;
        }
        rep[0] = nx[0]; rep[1] = nx[1]; rep[2] = nx[2];
        start += d->bprod;
    }
    frames[f].produced = start;
}

/* Fix.  grid: one single-wave workgroup per block, nblocks as for Entropy */
QZ_KERNEL_MAX(64) qzk_zstdd_bfix_kernel(const qzk_zdseg *segs, const qzk_zdplan *plan, const qzk_zdb_frame *frames, uint32_t nframes,
                                        uint32_t nblocks, qzk_zdb_desc *desc, uint8_t *scratch)
{
    const uint32_t lane = (uint32_t)qz_lane(), gb = blockIdx.x;
    if (gb >= nblocks) return;
    const qzk_zdb_frame *fr = frames + qzk_zdb_frame_of(frames, nframes, gb);
    const uint32_t b = gb - fr->first_blk;
    if (fr->decided || b >= fr->nblk) return;
    qzk_zdb_desc *const d = desc + gb;
    if (d->herr) return;
    const uint32_t nw = d->nrec, nseq = d->nseq, out_cap = segs[fr->seg].out_cap, bmax = fr->bmax;
    const qzk_zdplan pl = plan[fr->seg];
    if (nw == 0 || d->rec_pre >= pl.rec_cap || nw > pl.rec_cap - d->rec_pre) return;
    uint32_t *const rec = (uint32_t *)(scratch + pl.rec_off) + 3 * (size_t)d->rec_pre;
    const uint32_t r0 = d->rep_in[0], r1 = d->rep_in[1], r2 = d->rep_in[2];
    const uint64_t start = d->out_start;
    uint64_t base = start;
    for (uint32_t i0 = 0; i0 < nw; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool have = i < nw;
        uint32_t ll = 0, ml = 0, dist = 0;
        if (have) {
            uint32_t *p = rec + 3 * (size_t)i;
            ll = p[0]; ml = p[1]; dist = p[2];
            const uint32_t tag = ml >> 30;
            if (tag) {
                ml &= QZK_ZDB_MLMASK;
                dist = (tag == 1 ? r0 : tag == 2 ? r1 : r2) - dist;
                p[1] = ml; p[2] = dist;
            }
        }
        const uint32_t tot = ll + ml, incl = qz_wave_incl_scan(tot);
        const uint64_t before = base + (incl - tot), end = before + tot;
        int code = 0;
        if (have) {
            if (i < nseq) {
                if (dist == 0) code = QZK_ZD_EDATA;
                else if (end > out_cap) code = QZK_ZD_EOUT;
                else if ((uint64_t)dist > before + ll) code = QZK_ZD_EDATA;
            } else {
                /* the block's last record: its trailing literals, a Raw or an RLE block - and the block is whole */
                if (end > out_cap) code = QZK_ZD_EOUT;
                else if (end - start > bmax) code = QZK_ZD_EDATA;
                else if (fr->has_content && end > fr->content) code = QZK_ZD_EDATA;
            }
        }
        const uint64_t m = qz_ballot(code != 0);
        if (m != 0) {
            const int first = qz_ctz64(m);
            const uint32_t c = qz_shfl((uint32_t)code, first);
            if (lane == 0) { d->ferr = (int32_t)c; d->ferr_rec = i0 + (uint32_t)first; }
            return;
        }
        base += qz_shfl(incl, 63);
    }
}

/* Finish.  grid: one single-wave workgroup per routed frame */
QZ_KERNEL_MAX(64) qzk_zstdd_bfinish_kernel(const qzk_zdseg *segs, const qzk_zdb_frame *frames, uint32_t nframes, const qzk_zdb_desc *desc,
                                           qzk_zdres *res)
{
    const uint32_t f = blockIdx.x;
    if (f >= nframes || qz_lane() != 0) return;
    const qzk_zdb_frame fr = frames[f];
    const qzk_zdb_desc *const D = desc + fr.first_blk;
    int e = fr.status;
    uint32_t pos = fr.pos_end, nrec = 0;
    if (!fr.decided) {
        for (uint32_t b = 0; b < fr.nblk && !e; b++) {
            const qzk_zdb_desc *d = D + b;
            /* the header's refusals, then the earliest record: Fix looked at the records before the one Entropy stopped at */
            e = d->herr ? d->herr : d->ferr ? d->ferr : d->err;
            nrec = d->rec_pre + d->nseq + 1;
        }
        if (!e && !fr.complete) e = QZK_ZD_EDATA;                   /* (a walk that stops has left a refusal) */
        if (!e) {
            if (fr.has_content && fr.produced != fr.content) e = QZK_ZD_EDATA;
            else if (fr.has_cksum) { if (segs[fr.seg].in_len - pos < 4) e = QZK_ZD_ETRUNC; else pos += 4; }
        }
    }
    qzk_zdres o; o.status = e; o.in_used = e ? 0 : pos; o.out_len = e ? 0 : (uint32_t)fr.produced; o.pad = e ? 0 : nrec;
    res[fr.seg] = o;
}

#endif
