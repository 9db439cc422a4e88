/* inflate_plan_test.cpp - the decoder's host logic (qatzip_amd/csrc/qzd_inflate_plan.h) without a GPU: the seating sort, the
 * chain walk, the cut plan of a piece-wise decode and the pinned mirror's layout.  tests/test_inflate_plan.py compiles this
 * with the address and undefined-behaviour sanitizers and runs it; it exits 0 when every check holds. */
#include "qzd_inflate_plan.h"
#include <stdio.h>
#include <string.h>
#include <random>
#include <string>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

/* ---- seating ---- */
static void seating_case(const std::vector<uint32_t> &len, uint32_t shift)
{
    const uint32_t ns = (uint32_t)len.size();
    std::vector<uint32_t> start(ns);
    uint64_t n = 0;
    for (uint32_t i = 0; i < ns; i++) { start[i] = (uint32_t)n; n += len[i]; }
    for (uint32_t k = 0; k < ns; k++) CHECK(clen(start.data(), ns, n, k) == len[k]);
    std::vector<uint32_t> order(ns, 0xffffffffu), want(ns);
    order_by_clen(start, n, shift, order);
    auto cls = [&](uint32_t k) { return std::min<uint64_t>((uint64_t)len[k] >> shift, QZP_CLASSES - 1); };
    for (uint32_t i = 0; i < ns; i++) want[i] = i;
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return cls(a) > cls(b); });
    CHECK(order == want);
}
static void test_seating()
{
    std::mt19937 rng(20250523);
    const uint32_t sizes[] = {1, 2, 63, 64, 65, 5000};
    for (uint32_t shift : {5u, 8u})
        for (uint32_t ns : sizes) {
            std::vector<uint32_t> len(ns);
            /* lengths around a 64 KB segment's, a few tiny, a few equal: classes with several members */
            for (uint32_t i = 0; i < ns; i++) len[i] = rng() % 7 == 0 ? 1 + rng() % 64 : 20000 + rng() % 40000;
            if (ns == 5000) for (uint32_t i = 0; i < ns; i++) len[i] = std::min<uint32_t>(len[i], 400000u);      /* (the sum stays below 2^32) */
            seating_case(len, shift);
        }
    for (uint32_t shift : {5u, 8u}) {
        /* from QZP_CLASSES << shift on there is one class: those come first, in stream order */
        const uint32_t top = QZP_CLASSES << shift;
        const std::vector<uint32_t> len = {top - (1u << shift) - 1, top, 100, top + 12345, top * 3, top - 1, top + 1};    /* [0] is one class below */
        seating_case(len, shift);
        std::vector<uint32_t> start(len.size()), order(len.size());
        uint64_t n = 0;
        for (size_t i = 0; i < len.size(); i++) { start[i] = (uint32_t)n; n += len[i]; }
        order_by_clen(start, n, shift, order);
        CHECK((order == std::vector<uint32_t>{1, 3, 4, 5, 6, 0, 2}));
    }
    /* a piece seats only its own candidates: the last start is the next piece's, and bounds the one before it */
    {
        const std::vector<uint32_t> start = {0, 1000, 1100, 5000};
        std::vector<uint32_t> order(3);
        order_by_clen(start, 1 << 20, 5, order);
        CHECK((order == std::vector<uint32_t>{2, 0, 1}));
    }
    CHECK(cls_shift_of(NULL) == 8 && cls_shift_of("5") == 5 && cls_shift_of("0") == 0 && cls_shift_of("20") == 20);
    CHECK(cls_shift_of("21") == 8 && cls_shift_of("32") == 8 && cls_shift_of("-1") == 8 && cls_shift_of("x") == 0);
}

/* ---- chain walk ---- */
struct stream {                     /* candidates with their results, in stream order */
    std::vector<uint32_t> start; std::vector<qzp_res> res;
    void add(uint32_t at, int32_t status, uint32_t in_used, uint32_t out_len) { start.push_back(at); res.push_back(qzp_res{status, in_used, out_len, 1}); }
    qzp_walk walk(uint64_t cap = ~0ull, uint32_t want = 0, uint64_t oo = 0, uint32_t mine = ~0u, const uint32_t *where = NULL) const
    {
        return chain_walk(start.data(), (uint32_t)start.size(), std::min<uint32_t>(mine, (uint32_t)start.size()), res.data(), where, want, oo, cap);
    }
};
static bool same_links(const std::vector<qzp_link> &a, const std::vector<qzp_link> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) if (a[i].cand != b[i].cand || a[i].out_off != b[i].out_off || a[i].out_len != b[i].out_len) return false;
    return true;
}
static void test_walk()
{
    {   /* a clean chain to FINAL */
        stream s;
        s.add(0, QZP_FLUSH, 100, 1000); s.add(100, QZP_FLUSH, 50, 2000); s.add(150, QZP_FINAL, 30, 7);
        const qzp_walk W = s.walk();
        CHECK(W.ok && W.final && W.total_in == 180 && W.oo == 3007 && W.over == 3);
        CHECK(same_links(W.links, {{0, 0, 1000}, {1, 1000, 2000}, {2, 3000, 7}}));
    }
    {   /* a false candidate between two real ones drops out - whatever its own result says */
        for (int32_t st : {QZP_FLUSH, QZP_FINAL, -1, -4}) {
            stream s;
            s.add(0, QZP_FLUSH, 100, 1000); s.add(60, st, 10, 999); s.add(100, QZP_FINAL, 30, 7);
            const qzp_walk W = s.walk();
            CHECK(W.ok && W.final && W.total_in == 130 && W.oo == 1007);
            CHECK(same_links(W.links, {{0, 0, 1000}, {2, 1000, 7}}));
        }
    }
    {   /* a link that ends between two candidates, and one that ends behind the last */
        stream s;
        s.add(0, QZP_FLUSH, 80, 1000); s.add(60, QZP_FLUSH, 10, 999); s.add(100, QZP_FINAL, 30, 7);
        CHECK(!s.walk().ok && !s.walk().final);
        stream t;
        t.add(0, QZP_FLUSH, 100, 1000); t.add(100, QZP_FLUSH, 30, 7);
        CHECK(!t.walk().ok);
    }
    {   /* an error status on the chain */
        stream s;
        s.add(0, QZP_FLUSH, 100, 1000); s.add(100, -1, 50, 2000); s.add(150, QZP_FINAL, 30, 7);
        const qzp_walk W = s.walk();
        CHECK(!W.ok && W.links.size() == 1);
        s.res[1].status = 2;                                        /* (neither FLUSH nor FINAL) */
        CHECK(!s.walk().ok);
    }
    {   /* a `want` that is no candidate: between two, behind the last */
        stream s;
        s.add(0, QZP_FLUSH, 100, 1000); s.add(100, QZP_FINAL, 30, 7);
        CHECK(!s.walk(~0ull, 50).ok && s.walk(~0ull, 50).links.empty());
        CHECK(!s.walk(~0ull, 101).ok);
        CHECK(s.walk(~0ull, 100, 5).ok && s.walk(~0ull, 100, 5).oo == 12);
    }
    {   /* the cap: reported at the first link whose end lies beyond it, and not earlier */
        stream s;
        s.add(0, QZP_FLUSH, 100, 1000); s.add(100, QZP_FLUSH, 50, 2000); s.add(150, QZP_FLUSH, 10, 10); s.add(160, QZP_FINAL, 30, 7);
        CHECK(s.walk(3017).over == 4 && s.walk(3017).ok);
        CHECK(s.walk(3016).over == 3);
        CHECK(s.walk(3000).over == 2 && s.walk(3000).links.size() == 4 && s.walk(3000).ok);     /* the walk goes on: the policy is the caller's */
        CHECK(s.walk(2999).over == 1);
        CHECK(s.walk(1000).over == 1 && s.walk(999).over == 0 && s.walk(0).over == 0);
        s.res[2].status = -1;                                       /* ... also when the chain breaks behind it */
        CHECK(s.walk(2999).over == 1 && !s.walk(2999).ok);
        CHECK(s.walk(3000).over == 2 && !s.walk(3000).ok);          /* none: over == links.size() */
    }
    {   /* out of my candidates without FINAL: ok, not final, and where the chain goes on */
        stream s;
        s.add(0, QZP_FLUSH, 100, 1000); s.add(60, QZP_FLUSH, 1, 1); s.add(100, QZP_FLUSH, 50, 2000); s.add(150, QZP_FINAL, 30, 7);
        const qzp_walk W = s.walk(~0ull, 0, 0, 3);
        CHECK(W.ok && !W.final && W.next == 150 && W.oo == 3000 && W.links.size() == 2);
        const qzp_walk W0 = s.walk(~0ull, 0, 0, 0);                 /* a piece without a segment of its own */
        CHECK(W0.ok && !W0.final && W0.next == 0 && W0.oo == 0 && W0.links.empty());
    }
    {   /* a piece of qzd_inflate_stream_from_host sees one candidate beyond its own: when that one is no boundary the chain
         * does not close at the piece's end, and the pieces are abandoned */
        stream s;
        s.add(0, QZP_FLUSH, 100, 1000); s.add(60, QZP_FLUSH, 1, 1);
        CHECK(!s.walk(~0ull, 0, 0, 1).ok);
    }
    {   /* results through where[] */
        stream s;
        s.add(0, QZP_FLUSH, 100, 1000); s.add(100, QZP_FLUSH, 50, 2000); s.add(150, QZP_FINAL, 30, 7);
        const uint32_t where[3] = {2, 0, 1};
        std::swap(s.res[0], s.res[1]); std::swap(s.res[1], s.res[2]);       /* res[where[k]] = candidate k's */
        const qzp_walk W = s.walk(~0ull, 0, 0, ~0u, where);
        CHECK(W.ok && W.final && W.total_in == 180 && same_links(W.links, {{0, 0, 1000}, {1, 1000, 2000}, {2, 3000, 7}}));
    }
}
/* random chains with false candidates mixed in, walked whole and piece by piece with (want, oo) carried across every cut */
static void test_walk_pieces()
{
    std::mt19937 rng(4711);
    for (int round = 0; round < 200; round++) {
        stream s;
        const uint32_t nreal = 1 + rng() % 12;
        const int broken = round % 4 == 3 ? (int)(rng() % nreal) : -1;     /* a quarter of the chains break somewhere */
        uint32_t at = 0;
        for (uint32_t i = 0; i < nreal; i++) {
            const uint32_t used = 20 + rng() % 200, out = rng() % 70000;
            const bool fin = i + 1 == nreal;
            int32_t st = fin ? QZP_FINAL : QZP_FLUSH;
            uint32_t u = used;
            if ((int)i == broken) { if (rng() & 1) st = -1 - (int32_t)(rng() % 4); else u = used + 1 + rng() % 5; }
            s.add(at, st, u, out);
            for (uint32_t f = rng() % 3, q = at; f; f--) {          /* false candidates inside the segment, each with some result */
                q += 1 + rng() % 8;
                if (q >= at + used) break;
                s.add(q, (int32_t)(rng() % 6) - 4, rng() % 300, rng() % 70000);
            }
            at += used;
        }
        const uint32_t nc = (uint32_t)s.start.size();
        const qzp_walk whole = s.walk(100000);
        if (broken < 0) CHECK(whole.ok && whole.final && whole.total_in == at);
        /* piece p owns the candidates [b[p], b[p + 1]) and sees the later ones */
        for (uint32_t cut1 = 0; cut1 <= nc; cut1++)
            for (uint32_t cut2 = cut1; cut2 <= nc; cut2++) {
                const uint32_t b[4] = {0, cut1, cut2, nc};
                std::vector<qzp_link> links;
                uint32_t want = 0; uint64_t oo = 0, total_in = 0; bool ok = true, fin = false; size_t over = (size_t)-1;
                for (int p = 0; p < 3 && ok && !fin; p++) {
                    const bool last = p == 2;
                    const uint32_t lo = b[p], hi = nc;
                    if (lo >= hi) { if (last) ok = false; continue; }
                    const qzp_walk W = chain_walk(s.start.data() + lo, hi - lo, last ? hi - lo : b[p + 1] - lo, s.res.data() + lo, NULL, want, oo, 100000);
                    if (W.over < W.links.size() && over == (size_t)-1) over = links.size() + W.over;
                    for (qzp_link l : W.links) { l.cand += lo; links.push_back(l); }
                    ok = W.ok; fin = W.final; oo = W.oo; total_in = W.total_in; want = W.next;
                    if (ok && !fin && last) ok = false;
                }
                if (over == (size_t)-1) over = links.size();
                CHECK(ok == whole.ok && fin == whole.final && oo == whole.oo && total_in == whole.total_in && over == whole.over);
                CHECK(same_links(links, whole.links));
            }
    }
}

/* ---- the cut plan ---- */
static void check_cuts(const uint64_t *cut, uint32_t P, uint64_t n)
{
    CHECK(P >= 1 && P <= QZD_PIPE_MAX && cut[0] == 0 && cut[P] == n);
    for (uint32_t p = 1; p <= P; p++) CHECK(cut[p] >= cut[p - 1]);
    for (uint32_t p = 1; p < P; p++) CHECK(cut[p] % 4096 == 0);
}
static void test_pipe_plan()
{
    uint64_t cut[QZD_PIPE_MAX + 1]; uint32_t P = 0;
    const uint64_t MiB = 1 << 20;
    for (uint64_t n : {(uint64_t)1, (uint64_t)4095, 12 * MiB, 18 * MiB, 18 * MiB + 1, 24 * MiB, 100 * MiB + 17, 800 * MiB + 4097, (uint64_t)0xffffffffu}) {
        pipe_plan(n, cut, &P);
        check_cuts(cut, P, n);
        for (uint32_t p = 2; p < P; p++) CHECK(cut[p] - cut[p - 1] > cut[p - 1] - cut[p - 2]);      /* the pieces grow */
        if (P > 1 && P < QZD_PIPE_MAX) CHECK((cut[P] - cut[P - 1]) * 2 > cut[P - 1] - cut[P - 2]);  /* no tail under half its predecessor */
    }
    pipe_plan(18 * MiB, cut, &P);
    CHECK(P == 1);
    pipe_plan(18 * MiB + 1, cut, &P);
    CHECK(P == 2 && cut[1] == 12 * MiB);
    pipe_plan(0xffffffffu, cut, &P);
    CHECK(P == 6);                                                  /* 3 / 8 / 18 / 36 / 67 % */
    for (int want : {3, 8}) {
        const uint64_t n = 2 * MiB + 12345;
        pipe_plan_equal(n, want, cut, &P);
        CHECK(P == (uint32_t)want);
        check_cuts(cut, P, n);
        for (uint32_t p = 1; p < P; p++) CHECK(cut[p] == (n * p / P) / 4096 * 4096);
    }
    pipe_plan_equal(MiB, 100, cut, &P); CHECK(P == QZD_PIPE_MAX);
    pipe_plan_equal(MiB, 1, cut, &P); CHECK(P == 1 && cut[0] == 0 && cut[1] == MiB);
    pipe_plan_equal(MiB, -3, cut, &P); CHECK(P == 0);
    pipe_plan_equal(MiB, 0, cut, &P); CHECK(P == 0);
    {
        const uint64_t n = 100 * MiB;
        pipe_plan_equal(n, 3, cut, &P);
        pipe_cuts_percent(n, "10,40", P, cut); pipe_cuts_monotone(cut, P);
        CHECK(cut[0] == 0 && cut[1] == 10 * MiB && cut[2] == 40 * MiB && cut[3] == n);
        pipe_cuts_percent(n, "60,20", P, cut); pipe_cuts_monotone(cut, P);      /* descending: forced monotone */
        CHECK(cut[1] == 60 * MiB && cut[2] == 60 * MiB && cut[3] == n);
        check_cuts(cut, P, n);
        pipe_plan_equal(n, 4, cut, &P);
        pipe_cuts_percent(n, "10", P, cut); pipe_cuts_monotone(cut, P);         /* fewer values than boundaries: the rest stay */
        CHECK(cut[1] == 10 * MiB && cut[2] == 50 * MiB && cut[3] == 75 * MiB);
        pipe_cuts_percent(n, "1,2,3,4,5,6,7,8,9", P, cut); pipe_cuts_monotone(cut, P);  /* more values than boundaries: cut[P] stays */
        CHECK(cut[3] == 3 * MiB && cut[4] == n);
        pipe_cuts_percent(n, "150,-5,x", P, cut); pipe_cuts_monotone(cut, P);   /* out of range: clamped */
        CHECK(cut[1] == n && cut[2] == n && cut[3] == n && cut[4] == n);
        /* tiny cuts round down to nothing: a first piece of 8 KiB of a 2 MiB member */
        pipe_plan_equal(2 * MiB, 3, cut, &P);
        pipe_cuts_percent(2 * MiB, "1,2", P, cut); pipe_cuts_monotone(cut, P);
        CHECK(cut[1] == 20480 / 4096 * 4096 && cut[2] == 40960);
    }
}

/* ---- the mirror ---- */
static void test_mirror()
{
    for (uint32_t nsegs : {1u, 17u, 4096u})
        for (uint32_t K : {1u, 4u, 32u}) {
            const tp_mirror M = tp_mirror_of(nsegs, K);
            const size_t sb = (size_t)nsegs * sizeof(qzp_seg), rb = (size_t)nsegs * sizeof(qzp_res), tb = (size_t)nsegs * K * QZP_TOKSEG_BYTES;
            CHECK(M.o_res % 16 == 0 && M.o_ts % 16 == 0 && M.o_ord % 16 == 0);
            CHECK(sb <= M.o_res && M.o_res + rb <= M.o_ts && M.o_ts + tb <= M.o_ord && M.o_ord + (size_t)nsegs * 4 <= M.bytes);
        }
    CHECK(sizeof(qzp_seg) == 32 && sizeof(qzp_res) == 16);
}

int main()
{
    test_seating();
    test_walk();
    test_walk_pieces();
    test_pipe_plan();
    test_mirror();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("inflate_plan_test: ok\n");
    return 0;
}
