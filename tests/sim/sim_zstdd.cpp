/*
 * sim_zstdd.cpp — runs the zstd decode kernels (qatzip_amd/csrc/qzk_zstdd.h) on the CPU SIMT emulator (hipsim.h) behind a
 * C ABI for tests/test_sim_zstdd.py and tests/golden/gen_zstd_dec.py.  TEST INFRASTRUCTURE, as sim_driver.cpp.
 * The launch sequence is the device layer's (qzd_zstdd.hip, qzd_zstd_decompress_frames): rounds of frames by
 * qzd_zstdd_host.h itself, then per round stage E, stage X and the checksum kernel.
 * With SIM_ZSTDD_MAIN the file is a program of its own: `sim_zstdd refuse FILE...` expects a non-zero status of every file,
 * `sim_zstdd cut FILE` decodes the frame whole and cut at every byte, `sim_zstdd recipe BASE RECIPES OUT_CAP` decodes BASE once
 * per line "position value" of RECIPES with that byte set to that value and prints "position value status in_used out_len"
 * - each in an allocation of exactly its size, which is what a build with -fsanitize=address,undefined checks the loads
 * against.
 */
#define QZ_SIM 1
#include "hipsim.h"
#include "../../qatzip_amd/csrc/qzk_zstdd.h"
#include "../../qatzip_amd/csrc/qzd_zstdd_host.h"
#include <vector>

extern "C" {

uint32_t sim_zstdd_group(void) { return QZK_ZD_G; }

int64_t sim_zstdd_extent(const uint8_t *p, uint64_t n, uint64_t *content, int *has_content, uint64_t *bound, uint32_t *nblocks)
{
    bool hc = false;
    const int64_t r = qzd_zd_frame_walk(p, n, content, &hc, bound, nblocks);
    *has_content = hc;
    return r;
}

/* segs / res as qzd_zstd_decompress_frames takes them; out[0 .. out_size) is filled with 0xEE first and every byte of it
 * outside the segments' [out_off, out_off + out_cap) must still be 0xEE afterwards, like 64 bytes in front of and behind
 * each round's scratch and the spare rows between a frame's literals and its records: -3 otherwise.  scratch_cap 0: the
 * device layer's.  *rounds <- the rounds taken. */
int sim_zstdd_frames(const uint8_t *comp, const void *segs_v, uint32_t nsegs, uint8_t *out, uint64_t out_size, void *res_v,
                     uint64_t scratch_cap, uint32_t *rounds)
{
    const qzk_zdseg *segs = (const qzk_zdseg *)segs_v;
    qzk_zdres *res = (qzk_zdres *)res_v;
    if (!scratch_cap) scratch_cap = QZD_ZD_SCRATCH_CAP;
    memset(out, 0xEE, out_size);
    if (rounds) *rounds = 0;
    std::vector<qzk_zdplan> plan(nsegs ? nsegs : 1);
    int rc = 0;
    for (uint32_t first = 0; first < nsegs;) {
        uint64_t bytes = 0;
        const uint32_t k = qzd_zd_round(segs, first, nsegs, scratch_cap, plan.data(), &bytes);
        std::vector<uint8_t> scratch(bytes + 128, (uint8_t)0xEE);
        uint8_t *sc = scratch.data() + 64;
        const qzk_zdseg *sg = segs + first;
        qzk_zdres *rs = res + first;
        sim::launch((k + QZK_ZD_G - 1) / QZK_ZD_G, 64, 0, [&] { qzk_zstdd_entropy_kernel(comp, sg, plan.data(), rs, k, sc); });
        sim::launch(k, 64, 0, [&] { qzk_zstdd_exec_kernel(out, sg, plan.data(), rs, k, sc); });
        sim::launch(k, 64, 0, [&] { qzk_zstdd_xxh_kernel(comp, out, sg, rs, k); });
        for (size_t i = 0; i < 64; i++) if (scratch[i] != 0xEE || scratch[64 + bytes + i] != 0xEE) rc = -3;
        for (size_t i = 0; i < 16; i++) if (sc[i] != 0xEE || sc[bytes - 16 + i] != 0xEE) rc = -3;
        for (uint32_t j = 0; j < k; j++)
            for (uint64_t b = plan[j].lit_off + plan[j].lit_cap; b < plan[j].rec_off; b++) if (sc[b] != 0xEE) rc = -3;
        first += k;
        if (rounds) (*rounds)++;
    }
    std::vector<uint8_t> owned(out_size, 0);
    for (uint32_t i = 0; i < nsegs; i++)
        for (uint64_t b = 0; b < segs[i].out_cap && segs[i].out_off + b < out_size; b++) owned[segs[i].out_off + b] = 1;
    for (uint64_t b = 0; b < out_size; b++) if (!owned[b] && out[b] != 0xEE) rc = -3;
    return rc;
}

}

#ifdef SIM_ZSTDD_MAIN
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
static int decode_prefix(const std::vector<uint8_t> &frame, size_t n, uint32_t out_cap, qzk_zdres *r)
{
    uint8_t *in = (uint8_t *)malloc(n ? n : 1);
    memcpy(in, frame.data(), n);
    std::vector<uint8_t> out((size_t)out_cap + 128);
    qzk_zdseg sg; sg.in_off = 0; sg.out_off = 64; sg.in_len = (uint32_t)n; sg.out_cap = out_cap;
    const int rc = sim_zstdd_frames(in, &sg, 1, out.data(), out.size(), r, 0, NULL);
    free(in);
    return rc;
}
int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: sim_zstdd refuse|cut FILE... | recipe BASE RECIPES OUT_CAP\n"); return 2; }
    const bool cut = !strcmp(argv[1], "cut");
    int fails = 0;
    if (!strcmp(argv[1], "recipe")) {
        if (argc != 5) { fprintf(stderr, "usage: sim_zstdd recipe BASE RECIPES OUT_CAP\n"); return 2; }
        std::vector<uint8_t> frame = slurp(argv[2]);
        const uint32_t cap = (uint32_t)strtoul(argv[4], NULL, 10);
        FILE *f = fopen(argv[3], "r");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[3]); return 2; }
        unsigned long pos, value;
        while (fscanf(f, "%lu %lu", &pos, &value) == 2) {
            if (pos >= frame.size() || value > 255) { fprintf(stderr, "%s: byte %lu = %lu is outside the frame\n", argv[3], pos, value); fails++; continue; }
            const uint8_t keep = frame[pos];
            frame[pos] = (uint8_t)value;
            qzk_zdres r;
            const int rc = decode_prefix(frame, frame.size(), cap, &r);
            frame[pos] = keep;
            if (rc) { fprintf(stderr, "%s byte %lu = %lu: guard %d\n", argv[2], pos, value, rc); fails++; }
            printf("%lu %lu %d %u %u\n", pos, value, r.status, r.in_used, r.out_len);
        }
        fclose(f);
        printf("sim_zstdd: %d failures\n", fails);
        return fails ? 1 : 0;
    }
    for (int a = 2; a < argc; a++) {
        const std::vector<uint8_t> frame = slurp(argv[a]);
        uint64_t content = 0, bound = 0; bool hc = false;
        const int64_t ext = qzd_zd_frame_extent(frame.data(), frame.size(), &content, &hc, &bound);
        uint32_t cap = 4096;
        if (ext > 0) cap = (uint32_t)(hc ? content : bound);
        if (cap > (1u << 20)) cap = 1u << 20;
        qzk_zdres r;
        if (!cut) {
            const int rc = decode_prefix(frame, frame.size(), cap, &r);
            if (rc || r.status == 0) { fprintf(stderr, "%s: guard %d, status %d - a refusal was expected\n", argv[a], rc, r.status); fails++; }
            continue;
        }
        for (size_t n = 0; n <= frame.size(); n++) {
            const int rc = decode_prefix(frame, n, cap, &r);
            const bool whole = n == frame.size();
            if (rc || (r.status == 0) != whole || (whole && (r.in_used != n || r.out_len != content))) {
                fprintf(stderr, "%s cut at %zu: guard %d, status %d, in_used %u, out_len %u\n", argv[a], n, rc, r.status, r.in_used, r.out_len);
                fails++;
            }
        }
    }
    printf("sim_zstdd: %d failures\n", fails);
    return fails ? 1 : 0;
}
#endif
