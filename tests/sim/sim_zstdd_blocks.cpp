/*
 * sim_zstdd_blocks.cpp — runs the block route of the zstd decoder (qatzip_amd/csrc/qzk_zstdd_blocks.h) on the CPU SIMT
 * emulator (hipsim.h) behind a C ABI for tests/test_sim_zstdd_blocks.py and tests/golden/gen_zstd_dec_blocks.py.  TEST
 * INFRASTRUCTURE, as sim_zstdd.cpp.  The launch sequence is the device layer's (qzd_zstdd.hip,
 * qzd_zstd_decompress_frames_ex): rounds and routed frames by qzd_zstdd_host.h itself; per round stage E over the frames the
 * route leaves (a routed frame has no input there), Plan, Entropy, Scan, Fix and Finish over the routed ones, then stage X
 * and the checksum kernel over all of them.
 * With SIM_ZSTDDB_MAIN the file is a program of its own: `sim_zstdd_blocks FILE...` decodes every file under route `blocks`
 * (the count from the host's walk; where the walk fails, a count of 1, 2 and 40) and under route `frame` and expects the
 * same answer of both, `sim_zstdd_blocks cut FILE [FIRST LAST]` does so for the frame cut at every byte (at FIRST .. LAST
 * bytes), `sim_zstdd_blocks recipe BASE RECIPES OUT_CAP frame|blocks` decodes BASE once per line `position value count` of
 * RECIPES with that byte changed and that count, and prints `position value count status in_used out_len` - each input in
 * an allocation of exactly its size, which is what a build with -fsanitize=address,undefined checks the loads against.
 */
#define QZ_SIM 1
#include "hipsim.h"
#include "../../qatzip_amd/csrc/qzk_zstdd_blocks.h"
#include "../../qatzip_amd/csrc/qzd_zstdd_host.h"
#include <vector>

extern "C" {

uint32_t sim_zstddb_group(void) { return QZK_ZD_G; }
uint32_t sim_zstddb_min(void) { return QZD_ZD_BLOCKS_MIN; }
uint32_t sim_zstddb_desc_size(void) { return (uint32_t)sizeof(qzk_zdb_desc); }

/* as sim_zstdd_frames (sim_zstdd.cpp), with nblocks (may be NULL) and route as qzd_zstd_decompress_frames_ex and
 * qzd_zstd_decode_route take them.  *routed <- the frames that took the block route; *launches <- the kernels launched.  The
 * descriptors lie behind the round's scratch, guard bytes behind them. */
/* fail_blk (may be NULL): per segment the earliest block of a routed frame that Finish found refused, -1 where the frame is
 * not routed, is accepted or is refused as a whole (its header, its count, its content size, its checksum) */
int sim_zstddb_frames_fb(const uint8_t *comp, const void *segs_v, uint32_t nsegs, uint8_t *out, uint64_t out_size, void *res_v,
                         const uint32_t *nblocks, int route, uint64_t scratch_cap, uint32_t *rounds, uint32_t *routed, uint32_t *launches,
                         int32_t *fail_blk)
{
    const qzk_zdseg *segs = (const qzk_zdseg *)segs_v;
    qzk_zdres *res = (qzk_zdres *)res_v;
    if (!scratch_cap) scratch_cap = QZD_ZD_SCRATCH_CAP;
    memset(out, 0xEE, out_size);
    if (rounds) *rounds = 0;
    if (routed) *routed = 0;
    if (launches) *launches = 0;
    if (route == 1) nblocks = NULL;
    for (uint32_t i = 0; fail_blk && i < nsegs; i++) fail_blk[i] = -1;
    std::vector<qzk_zdplan> plan(nsegs ? nsegs : 1);
    std::vector<qzk_zdb_frame> fr(nsegs ? nsegs : 1);
    int rc = 0;
    for (uint32_t first = 0; first < nsegs;) {
        uint64_t bytes = 0, nblk = 0;
        const uint32_t k = qzd_zd_round(segs, first, nsegs, scratch_cap, plan.data(), &bytes);
        const uint32_t nfr = qzd_zdb_round(segs, nblocks, first, k, route, fr.data(), &nblk);
        const uint64_t desc_off = (bytes + 15) & ~15ull, all = nfr ? desc_off + qzd_zdb_desc_bytes(nblk) : bytes;
        std::vector<uint8_t> scratch(all + 128, (uint8_t)0xEE);
        uint8_t *sc = scratch.data() + 64;
        const qzk_zdseg *sg = segs + first;
        qzk_zdres *rs = res + first;
        std::vector<qzk_zdseg> esegs(sg, sg + k);
        for (uint32_t j = 0; j < nfr; j++) esegs[fr[j].seg].in_len = 0;
        uint32_t nl = 0;
        if (nfr < k) { sim::launch((k + QZK_ZD_G - 1) / QZK_ZD_G, 64, 0, [&] { qzk_zstdd_entropy_kernel(comp, esegs.data(), plan.data(), rs, k, sc); }); nl++; }
        if (nfr) {
            qzk_zdb_desc *desc = (qzk_zdb_desc *)(sc + desc_off);
            const uint32_t nb = (uint32_t)nblk;
            sim::launch(nfr, 64, 0, [&] { qzk_zstdd_bplan_kernel(comp, sg, plan.data(), fr.data(), nfr, desc, (uint32_t *)NULL); });
            sim::launch((nb + QZK_ZD_G - 1) / QZK_ZD_G, 64, 0, [&] { qzk_zstdd_bentropy_kernel(comp, sg, plan.data(), fr.data(), nfr, nb, desc, sc); });
            sim::launch(nfr, 64, 0, [&] { qzk_zstdd_bscan_kernel(fr.data(), nfr, desc); });
            sim::launch(nb, 64, 0, [&] { qzk_zstdd_bfix_kernel(sg, plan.data(), fr.data(), nfr, nb, desc, sc); });
            sim::launch(nfr, 64, 0, [&] { qzk_zstdd_bfinish_kernel(sg, fr.data(), nfr, desc, rs); });
            nl += 5;
            for (uint32_t j = 0; fail_blk && j < nfr; j++) {
                const qzk_zdb_frame &f = fr[j];
                for (uint32_t b = 0; !f.decided && b < f.nblk; b++) {
                    const qzk_zdb_desc &d = desc[f.first_blk + b];
                    if (d.herr || d.ferr || d.err) { fail_blk[first + f.seg] = (int32_t)b; break; }
                }
            }
        }
        sim::launch(k, 64, 0, [&] { qzk_zstdd_exec_kernel(out, sg, plan.data(), rs, k, sc); });
        sim::launch(k, 64, 0, [&] { qzk_zstdd_xxh_kernel(comp, out, sg, rs, k); });
        nl += 2;
        for (size_t i = 0; i < 64; i++) if (scratch[i] != 0xEE || scratch[64 + all + i] != 0xEE) rc = -3;
        for (size_t i = 0; i < 16; i++) if (sc[i] != 0xEE || sc[bytes - 16 + i] != 0xEE) rc = -3;
        for (uint32_t j = 0; j < k; j++)
            for (uint64_t b = plan[j].lit_off + plan[j].lit_cap; b < plan[j].rec_off; b++) if (sc[b] != 0xEE) rc = -3;
        first += k;
        if (rounds) (*rounds)++;
        if (routed) *routed += nfr;
        if (launches) *launches += nl;
    }
    std::vector<uint8_t> owned(out_size, 0);
    for (uint32_t i = 0; i < nsegs; i++)
        for (uint64_t b = 0; b < segs[i].out_cap && segs[i].out_off + b < out_size; b++) owned[segs[i].out_off + b] = 1;
    for (uint64_t b = 0; b < out_size; b++) if (!owned[b] && out[b] != 0xEE) rc = -3;
    return rc;
}

int sim_zstddb_frames(const uint8_t *comp, const void *segs_v, uint32_t nsegs, uint8_t *out, uint64_t out_size, void *res_v,
                      const uint32_t *nblocks, int route, uint64_t scratch_cap, uint32_t *rounds, uint32_t *routed, uint32_t *launches)
{
    return sim_zstddb_frames_fb(comp, segs_v, nsegs, out, out_size, res_v, nblocks, route, scratch_cap, rounds, routed, launches, NULL);
}

/* qzd_zstd_count_blocks: the Plan walk without descriptors */
void sim_zstddb_count(const uint8_t *comp, const void *segs_v, uint32_t nsegs, uint32_t *counts)
{
    const qzk_zdseg *segs = (const qzk_zdseg *)segs_v;
    std::vector<qzk_zdb_frame> fr(nsegs ? nsegs : 1);
    memset(fr.data(), 0, fr.size() * sizeof(qzk_zdb_frame));
    for (uint32_t i = 0; i < nsegs; i++) { fr[i].seg = i; fr[i].hint = 0xffffffffu; }
    sim::launch(nsegs, 64, 0, [&] { qzk_zstdd_bplan_kernel(comp, segs, (const qzk_zdplan *)NULL, fr.data(), nsegs, (qzk_zdb_desc *)NULL, counts); });
}

}

#ifdef SIM_ZSTDDB_MAIN
static std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}
/* the first n bytes of the frame, alone in an allocation of n bytes; out_cap bytes of output between guards */
static int decode_prefix(const std::vector<uint8_t> &frame, size_t n, uint32_t out_cap, uint32_t nblocks, int route, qzk_zdres *r, std::vector<uint8_t> *o)
{
    uint8_t *in = (uint8_t *)malloc(n ? n : 1);
    memcpy(in, frame.data(), n);
    std::vector<uint8_t> out((size_t)out_cap + 128);
    qzk_zdseg sg; sg.in_off = 0; sg.out_off = 64; sg.in_len = (uint32_t)n; sg.out_cap = out_cap;
    const int rc = sim_zstddb_frames(in, &sg, 1, out.data(), out.size(), r, &nblocks, route, 0, NULL, NULL, NULL);
    free(in);
    if (o) o->assign(out.begin() + 64, out.begin() + 64 + (r->status == 0 ? r->out_len : 0));
    return rc;
}
static int both(const char *name, const std::vector<uint8_t> &frame, size_t n, uint32_t cap)
{
    uint64_t content = 0, bound = 0; bool hc = false; uint32_t nb = 0;
    const int64_t ext = qzd_zd_frame_walk(frame.data(), n, &content, &hc, &bound, &nb);
    const uint32_t tries[3] = { 1, 2, 40 };
    int fails = 0;
    qzk_zdres a, b;
    std::vector<uint8_t> oa, ob;
    int rc = decode_prefix(frame, n, cap, 0, 1, &a, &oa);
    if (rc) { fprintf(stderr, "%s at %zu, route frame: guard %d\n", name, n, rc); fails++; }
    for (uint32_t t = 0; t < (ext > 0 && nb ? 1u : 3u); t++) {
        const uint32_t hint = ext > 0 && nb ? nb : tries[t];
        rc = decode_prefix(frame, n, cap, hint, 2, &b, &ob);
        const bool same = (b.status == QZK_ZD_EHINT && a.status != 0 && !(ext > 0 && nb)) ||
                          (a.status == b.status && a.in_used == b.in_used && a.out_len == b.out_len && oa == ob);
        if (rc || !same) {
            fprintf(stderr, "%s at %zu, count %u: guard %d, blocks {%d, %u, %u}, frame {%d, %u, %u}\n", name, n, hint, rc, b.status, b.in_used, b.out_len,
                    a.status, a.in_used, a.out_len);
            fails++;
        }
    }
    return fails;
}
int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: sim_zstdd_blocks FILE... | cut FILE [FIRST LAST] | recipe BASE RECIPES OUT_CAP frame|blocks\n"); return 2; }
    const bool cut = !strcmp(argv[1], "cut");
    int fails = 0;
    if (!strcmp(argv[1], "recipe")) {
        if (argc != 6 || (strcmp(argv[5], "frame") && strcmp(argv[5], "blocks"))) { fprintf(stderr, "usage: sim_zstdd_blocks recipe BASE RECIPES OUT_CAP frame|blocks\n"); return 2; }
        std::vector<uint8_t> frame = slurp(argv[2]);
        const uint32_t cap = (uint32_t)strtoul(argv[4], NULL, 10);
        const int route = !strcmp(argv[5], "frame") ? 1 : 2;
        FILE *f = fopen(argv[3], "r");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[3]); return 2; }
        unsigned long pos, value, count;
        while (fscanf(f, "%lu %lu %lu", &pos, &value, &count) == 3) {
            if (pos >= frame.size() || value > 255) { fprintf(stderr, "%s: byte %lu = %lu is outside the frame\n", argv[3], pos, value); fails++; continue; }
            const uint8_t keep = frame[pos];
            frame[pos] = (uint8_t)value;
            qzk_zdres r;
            const int rc = decode_prefix(frame, frame.size(), cap, (uint32_t)count, route, &r, NULL);
            frame[pos] = keep;
            if (rc) { fprintf(stderr, "%s byte %lu = %lu, count %lu: guard %d\n", argv[2], pos, value, count, rc); fails++; }
            printf("%lu %lu %lu %d %u %u\n", pos, value, count, r.status, r.in_used, r.out_len);
        }
        fclose(f);
        printf("sim_zstdd_blocks: %d failures\n", fails);
        return fails ? 1 : 0;
    }
    if (cut && argc != 3 && argc != 5) { fprintf(stderr, "usage: sim_zstdd_blocks cut FILE [FIRST LAST]\n"); return 2; }
    for (int a = cut ? 2 : 1; a < (cut ? 3 : argc); a++) {
        const std::vector<uint8_t> frame = slurp(argv[a]);
        uint64_t content = 0, bound = 0; bool hc = false;
        const int64_t ext = qzd_zd_frame_extent(frame.data(), frame.size(), &content, &hc, &bound);
        uint32_t cap = 4096;
        if (ext > 0) cap = (uint32_t)(hc ? content : bound);
        if (cap > (1u << 20)) cap = 1u << 20;
        if (!cut) fails += both(argv[a], frame, frame.size(), cap);
        else {
            size_t lo = 0, hi = frame.size();
            if (argc == 5) { lo = strtoul(argv[3], NULL, 10); hi = strtoul(argv[4], NULL, 10); if (hi > frame.size()) hi = frame.size(); }
            for (size_t n = lo; n <= hi; n++) fails += both(argv[a], frame, n, cap);
        }
    }
    printf("sim_zstdd_blocks: %d failures\n", fails);
    return fails ? 1 : 0;
}
#endif
