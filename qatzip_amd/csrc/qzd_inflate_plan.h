/* qzd_inflate_plan.h — the decoder's host logic that needs no GPU: the seating of candidates by compressed size, the chain
 * walk (the one place where untrusted input decides output offsets), the cut plan of a piece-wise decode and the layout of
 * two_phase()'s pinned mirror.  Plain C++17, no HIP header and no qzd_ctx: tests/c/inflate_plan_test.cpp includes only this
 * file and runs it under the address and undefined-behaviour sanitizers. */
#ifndef QZD_INFLATE_PLAN_H
#define QZD_INFLATE_PLAN_H
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

/* mirrors of qzk_infseg / qzk_infres (qzk_inflate.h); qzd_inflate.hip holds the static_asserts that keep them in step */
struct qzp_seg { uint64_t in_off, out_off; uint32_t in_len, out_cap, flags, pad; };
struct qzp_res { int32_t status; uint32_t in_used, out_len, nblocks; };
#define QZP_FINAL 0                 /* QZK_INF_FINAL */
#define QZP_FLUSH 1                 /* QZK_INF_FLUSH */
#define QZP_TOKSEG_BYTES 16u        /* sizeof(qzk_tokseg) */

/* compressed length of candidate k at most: up to the next candidate's start, the last one's to the end of the n bytes */
static inline uint32_t clen(const uint32_t *start, uint32_t ns, uint64_t n, uint32_t k)
{
    return (k + 1 < ns ? start[k + 1] : (uint32_t)n) - start[k];
}

/* The seating: order[0 .. order.size()) = the first order.size() candidates by compressed length, largest class first (the
 * segments with the most symbols are the critical path, so their waves start first), a class in stream order.  A stable
 * counting sort over QZP_CLASSES classes of (1 << shift) bytes - lengths from QZP_CLASSES << shift on share the last one:
 * grouping only needs "similar", and an exact sort would seat byte-identical segments (tiled test data) in the same wave,
 * where they never diverge. */
#define QZP_CLASSES 8192u
static inline void order_by_clen(const std::vector<uint32_t> &start, uint64_t n, uint32_t shift, std::vector<uint32_t> &order)
{
    const uint32_t ns = (uint32_t)order.size(), nstart = (uint32_t)start.size();
    std::vector<uint32_t> cnt(QZP_CLASSES + 1, 0);
    auto rcls = [&](uint32_t k) { const uint32_t v = clen(start.data(), nstart, n, k) >> shift; return QZP_CLASSES - 1 - (v < QZP_CLASSES ? v : QZP_CLASSES - 1); };
    for (uint32_t i = 0; i < ns; i++) cnt[rcls(i) + 1]++;
    for (uint32_t i = 0; i < QZP_CLASSES; i++) cnt[i + 1] += cnt[i];
    for (uint32_t i = 0; i < ns; i++) order[cnt[rcls(i)]++] = i;
}
/* QATZIP_AMD_INFLATE_CLS=<log2 of the class>: 0 .. 20, anything else (or nothing) means 256-byte classes */
static inline uint32_t cls_shift_of(const char *env)
{
    const int v = env ? atoi(env) : 8;
    return v >= 0 && v <= 20 ? (uint32_t)v : 8u;
}

/* The chain walk.  start[0 .. nstart) are the sorted candidate starts, the first `mine` of them have a result (candidate k's
 * is res[where ? where[k] : k]).  From the candidate that starts at `want`, with the output at `oo`: every link must have ended
 * at a flush marker or in the final block, and must end exactly where another candidate starts - candidates in between are
 * no boundaries (00 00 FF FF inside compressed data) and drop out.  The walk ends at the final block, at the first
 * candidate that is not mine (ok, not final: `next` is where the chain goes on), or where the chain breaks (not ok). */
struct qzp_link { uint32_t cand; uint64_t out_off; uint32_t out_len; };
struct qzp_walk {
    std::vector<qzp_link> links;    /* the real segments, in output order */
    bool ok, final;
    uint64_t total_in;              /* final: the stream's compressed bytes */
    uint64_t oo;                    /* the output offset reached */
    uint32_t next;                  /* ok and not final: the start the chain expects next */
    size_t over;                    /* the first link whose end lies beyond `cap`; links.size() if none does */
};
static inline qzp_walk chain_walk(const uint32_t *start, uint32_t nstart, uint32_t mine, const qzp_res *res, const uint32_t *where,
                                  uint32_t want, uint64_t oo, uint64_t cap)
{
    qzp_walk W;
    W.ok = true; W.final = false; W.total_in = 0; W.next = want; W.over = (size_t)-1;
    uint32_t k = 0;                                                 /* the starts are sorted and the expected one only grows */
    while (k < nstart && start[k] < want) k++;
    if (k >= nstart || start[k] != want) W.ok = false;
    while (W.ok && k < mine) {
        const qzp_res &r = res[where ? where[k] : k];
        if (r.status != QZP_FINAL && r.status != QZP_FLUSH) { W.ok = false; break; }
        W.links.push_back(qzp_link{k, oo, r.out_len});
        oo += r.out_len;
        if (oo > cap && W.over == (size_t)-1) W.over = W.links.size() - 1;
        if (r.status == QZP_FINAL) { W.final = true; W.total_in = (uint64_t)start[k] + r.in_used; break; }
        W.next = start[k] + r.in_used;
        uint32_t j = k + 1;
        while (j < nstart && start[j] < W.next) j++;
        if (j >= nstart || start[j] != W.next) { W.ok = false; break; }
        k = j;
    }
    W.oo = oo;
    if (W.over == (size_t)-1) W.over = W.links.size();
    return W;
}

/* ---- the cut plan of a piece-wise decode (qzd_inflate_stream_from_host): cut[0] = 0 <= cut[1] <= ... <= cut[P] = n ----
 * The pieces GROW: the output cannot leave before the first piece has been through both phases, and a launch of phase A
 * lasts as long as its slowest segment however few there are (3.8 ms for 16 MiB or 64) - so the first piece is small, 3 % of
 * the member, and every later one is as much larger as the link needs to stay busy: piece p + 1 must be decoded when piece
 * p has left.  Round 5 (profiles/r5_api_decompress_pieces.txt, 2047 MiB): two pieces cut at a third 53.5 ms, four equal ones
 * 50.1, six cut at 3 / 8 / 17 / 33 / 60 % 47.3 = 45.3 GB/s, 0.80 of the link.  (Rounds 4's finding that more pieces lose was
 * made with helpers that shared hardware queues: see stream_own_queue in qzd_device.hip.) */
#define QZD_PIPE_MAX 8u
#define QZD_PIPE_FIRST_PCT 3u              /* the first piece, percent of the member ... */
#define QZD_PIPE_MIN_BYTES (12u << 20)     /* ... but this many compressed bytes at least (~32 MiB of output, 512 segments) */
#define QZD_PIPE_GROW_NUM 9u               /* every piece 1.8 times the one before */
#define QZD_PIPE_GROW_DEN 5u
static inline void pipe_plan(uint64_t n, uint64_t cut[QZD_PIPE_MAX + 1], uint32_t *P_out)
{
    uint64_t len = std::max<uint64_t>(n * QZD_PIPE_FIRST_PCT / 100, QZD_PIPE_MIN_BYTES), at = 0;
    uint32_t P = 0;
    cut[0] = 0;
    while (P + 1 < QZD_PIPE_MAX && at + len + len / 2 < n) {        /* (a last piece smaller than half its predecessor joins it) */
        at = (at + len) & ~(uint64_t)4095; cut[++P] = at;
        len = len * QZD_PIPE_GROW_NUM / QZD_PIPE_GROW_DEN;
    }
    cut[++P] = n;
    *P_out = P;
}
/* QATZIP_AMD_PIPE=<pieces>: that many equal ones (0 / 1: the whole member at once) */
static inline void pipe_plan_equal(uint64_t n, int pieces, uint64_t cut[QZD_PIPE_MAX + 1], uint32_t *P_out)
{
    const uint32_t P = (uint32_t)std::min<int>(QZD_PIPE_MAX, std::max(0, pieces));
    for (uint32_t p = 0; p <= P; p++) cut[p] = p == P ? n : (n * p / P) & ~(uint64_t)4095;
    *P_out = P;
}
/* QATZIP_AMD_PIPE_CUTS="10,40": the interior boundaries of P pieces in percent of the member (developer aid) */
static inline void pipe_cuts_percent(uint64_t n, const char *pcts, uint32_t P, uint64_t cut[QZD_PIPE_MAX + 1])
{
    uint32_t k = 1;
    for (const char *q = pcts; *q && k < P; k++) {
        cut[k] = (n * (uint64_t)std::min(100, std::max(0, atoi(q))) / 100) & ~(uint64_t)4095;
        while (*q && *q != ',') q++;
        if (*q) q++;
    }
}
static inline void pipe_cuts_monotone(uint64_t cut[QZD_PIPE_MAX + 1], uint32_t P)
{
    for (uint32_t p = 1; p <= P; p++) if (cut[p] < cut[p - 1]) cut[p] = cut[p - 1];      /* boundaries only ever go up */
}

/* The pinned mirror of the aux scratch as two_phase() lays it out for nsegs segments with K sub-streams each, and as
 * two_phase_resolve() finds it again (c->tp holds that call's nsegs and K): the segment records at 0, the results at o_res,
 * the sub-stream descriptors at o_ts, a list of nsegs indices at o_ord; `bytes` holds them all. */
struct tp_mirror { size_t o_res, o_ts, o_ord, bytes; };
static inline tp_mirror tp_mirror_of(uint32_t nsegs, uint32_t K)
{
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    tp_mirror M;
    M.o_res = up16((size_t)nsegs * sizeof(qzp_seg));
    M.o_ts = M.o_res + up16((size_t)nsegs * sizeof(qzp_res));
    M.o_ord = M.o_ts + up16((size_t)nsegs * K * QZP_TOKSEG_BYTES);
    M.bytes = M.o_ord + (size_t)nsegs * 4;
    return M;
}

#endif
