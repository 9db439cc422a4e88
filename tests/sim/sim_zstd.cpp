/*
 * sim_zstd.cpp — runs the zstd kernels (qatzip_amd/csrc/qzk_zstd.h) on the CPU SIMT emulator (hipsim.h) behind a C ABI for
 * tests/test_sim_zstd.py and tests/golden/gen_zstd.py.  TEST INFRASTRUCTURE, as sim_driver.cpp.
 * The launch sequences are the device layer's (qzd_device.hip, qzd_zstd_compress_frames / qzd_zstd_encode_frames): the host
 * side of them - the bound, the frame descriptions, the scan over the frame lengths - is qzd_zstd_host.h itself; gather is
 * restated in plain C++ (it is not a kernel of a header).
 * With SIM_ZSTD_MAIN the file is a program of its own that runs the edge list of tests/test_sim_zstd.py's encode_frames
 * cases through that host side: what a build with -fsanitize=address,undefined runs.
 */
#define QZ_SIM 1
#include "hipsim.h"
#include "../../qatzip_amd/csrc/qzk_zstd.h"
#include "../../qatzip_amd/csrc/qzd_zstd_host.h"
#include <vector>

/* slots filled with 0xEE, 64 guard bytes behind bound + slack that must still be 0xEE afterwards; every frame within its
 * bound: -3 otherwise.  -1: out_cap does not hold the result. */
static int collect(const std::vector<uint8_t> &slots, uint32_t stride, const std::vector<uint32_t> &lens, const std::vector<uint32_t> &content,
                   uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *frame_len)
{
    std::vector<uint64_t> offs(lens.size());
    const uint64_t total = qzd_zs_scan(lens.data(), (uint32_t)lens.size(), offs.data());
    for (size_t i = 0; i < lens.size(); i++) {
        if (lens[i] > QZK_ZS_BOUND(content[i])) return -3;
        for (uint32_t k = QZK_ZS_BOUND(content[i]) + QZK_ZS_SLACK; k < stride; k++) if (slots[i * stride + k] != 0xEE) return -3;
        if (offs[i] + lens[i] > out_cap) return -1;
        memcpy(out + offs[i], slots.data() + i * stride, lens[i]);
        if (frame_len) frame_len[i] = lens[i];
    }
    *out_len = total;
    return 0;
}

extern "C" {

uint64_t sim_zstd_bound(uint64_t n, uint32_t block_sz) { return qzd_zs_bound(n, block_sz); }

/* every block_sz bytes of src a frame, by `waves` persistent waves (0: one per chunk).  Returns 0, -1, -2 for bad
 * parameters, -3 (see collect). */
int sim_zstd(const uint8_t *src, uint64_t total, uint32_t block_sz, uint32_t mini_match, uint32_t waves,
             uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *frame_len)
{
    if (!qzd_zs_params_ok(block_sz, mini_match)) return -2;
    *out_len = 0;
    if (!total) return 0;
    const uint32_t nb = (uint32_t)((total + block_sz - 1) / block_sz);
    const uint32_t stride = qzd_zs_stride(block_sz) + 64;
    std::vector<uint8_t> slots((size_t)nb * stride, (uint8_t)0xEE);
    std::vector<uint32_t> lens(nb), content(nb);
    for (uint32_t i = 0; i < nb; i++) content[i] = (uint32_t)(total - (uint64_t)i * block_sz < block_sz ? total - (uint64_t)i * block_sz : block_sz);
    uint32_t counter = 0;
    if (!waves || waves > nb) waves = nb;
    std::vector<uint8_t> scratch((size_t)waves * QZK_ZS_WAVEB(block_sz) + 64, (uint8_t)0xEE);
    sim::launch(waves, 64, 0, [&] { qzk_zstd_pull_kernel(src, total, block_sz, nb, slots.data(), stride, lens.data(), mini_match, &counter, scratch.data()); });
    for (size_t k = (size_t)waves * QZK_ZS_WAVEB(block_sz); k < scratch.size(); k++) if (scratch[k] != 0xEE) return -3;
    return collect(slots, stride, lens, content, out, out_cap, out_len, frame_len);
}

/* the entropy stage alone: desc = nframes x (content size, records, literals), records and literals back to back in frame
 * order.  Returns 0, -1, -3, or the device layer's answer to a description or to records it refuses: -10 for QZD_ERR_PARAM,
 * -11 for QZD_ERR_DATA. */
int sim_zstd_encode(const uint8_t *lits, const uint32_t *seqs, const uint32_t *desc, uint32_t nframes, uint32_t waves,
                    uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *frame_len)
{
    *out_len = 0;
    if (!nframes) return 0;
    std::vector<qzk_zs_fdesc> fd(nframes);
    uint32_t maxc = 0;
    if (!qzd_zs_describe(desc, nframes, fd.data(), &maxc, NULL, NULL)) return -10;
    const uint32_t stride = qzd_zs_stride(maxc) + 64;
    std::vector<uint8_t> slots((size_t)nframes * stride, (uint8_t)0xEE);
    std::vector<uint32_t> lens(nframes), content(nframes);
    for (uint32_t i = 0; i < nframes; i++) content[i] = fd[i].content;
    uint32_t counter = 0, bad = 0;
    if (!waves || waves > nframes) waves = nframes;
    sim::launch(waves, 64, 0, [&] { qzk_zstd_encode_kernel(lits, (const qzk_zs_seq *)seqs, fd.data(), nframes, slots.data(), stride, lens.data(), &bad, &counter); });
    if (bad) return -11;
    return collect(slots, stride, lens, content, out, out_cap, out_len, frame_len);
}

}

#ifdef SIM_ZSTD_MAIN
/* the edge list: per case a frame of `nl` literals (byte i is (i * mul) % mod) and `ns` records (ll, ml, off); the answer
 * expected of the host side and the kernel together */
struct Case { uint32_t content, nl, mod, ns, ll, ml, off; int expect; };
static int run_case(const Case &k)
{
    std::vector<uint8_t> lits(k.nl + 1);
    for (uint32_t i = 0; i < k.nl; i++) lits[i] = (uint8_t)((i * 7u) % k.mod);
    std::vector<uint32_t> seqs(3 * (size_t)k.ns + 3);
    for (uint32_t i = 0; i < k.ns; i++) { seqs[3 * i] = k.ll; seqs[3 * i + 1] = k.ml; seqs[3 * i + 2] = k.off; }
    const uint32_t desc[3] = { k.content, k.ns, k.nl };
    std::vector<uint8_t> out(qzd_zs_bound(k.content <= QZK_ZS_MAXBLK ? k.content : 0, QZK_ZS_MAXBLK) + 64);
    uint64_t ol = 0; uint32_t fl = 0;
    const int rc = sim_zstd_encode(lits.data(), seqs.data(), desc, 1, 0, out.data(), out.size(), &ol, &fl);
    if (rc != k.expect) { fprintf(stderr, "case content=%u nl=%u ns=%u: rc %d, expected %d\n", k.content, k.nl, k.ns, rc, k.expect); return 1; }
    if (rc == 0 && (ol != fl || ol > qzd_zs_bound(k.content, QZK_ZS_MAXBLK))) { fprintf(stderr, "case content=%u: length %llu\n", k.content, (unsigned long long)ol); return 1; }
    return 0;
}
int main()
{
    static const Case cases[] = {
        { 31, 31, 251, 0, 0, 0, 0, 0 }, { 32, 32, 251, 0, 0, 0, 0, 0 }, { 4095, 4095, 251, 0, 0, 0, 0, 0 }, { 4096, 4096, 256, 0, 0, 0, 0, 0 },
        { 1023, 1023, 5, 0, 0, 0, 0, 0 }, { 1024, 1024, 5, 0, 0, 0, 0, 0 }, { 16383, 16383, 5, 0, 0, 0, 0, 0 }, { 16384, 16384, 200, 0, 0, 0, 0, 0 },
        { 100, 100, 1, 0, 0, 0, 0, 0 }, { 5000, 5000, 2, 0, 0, 0, 0, 0 },
        { 1 + 4, 1, 7, 1, 1, 4, 1, 0 }, { 127 * 4, 127, 7, 127, 1, 3, 1, 0 }, { 128 * 4, 128, 7, 128, 1, 3, 1, 0 },
        { 0x7eff * 4, 0x7eff, 7, 0x7eff, 1, 3, 1, 0 }, { 0x7f00 * 4, 0x7f00, 7, 0x7f00, 1, 3, 1, 0 },
        { 65536 + 65535, 65536, 251, 1, 65536, 65535, 65535, 0 }, { 131072, 131069, 251, 1, 131069, 3, 5, 0 },
        { 131073, 131070, 251, 1, 131070, 3, 5, -10 },              /* content above 128 KB */
        { 10, 4, 7, 1, 4, 5, 1, -11 },                              /* lengths do not add up */
        { 9, 4, 7, 1, 4, 5, 0, -11 }, { 9, 4, 7, 1, 4, 5, 5, -11 }, /* offset 0, offset beyond the bytes produced */
        { 6, 4, 7, 1, 4, 2, 1, -10 },                               /* a match shorter than 3: more records than a third of what they cover */
        { 9, 3, 7, 1, 4, 5, 1, -11 },                               /* more literals taken than there are */
        { 6, 7, 7, 0, 0, 0, 0, -10 }, { 6, 0, 7, 3, 0, 3, 1, -10 }, { 0, 0, 7, 0, 0, 0, 0, -10 },
    };
    int fails = 0;
    for (const Case &k : cases) fails += run_case(k);
    /* the frame-length scan and the bound over a call's chunks */
    const uint32_t lens[5] = { 12, 0, 131084, 7, 1 }; uint64_t offs[5];
    if (qzd_zs_scan(lens, 5, offs) != 131104 || offs[4] != 131103 || offs[1] != 12) { fprintf(stderr, "scan\n"); fails++; }
    if (qzd_zs_bound(300000, 131072) != 300000 + 3 * 12 || qzd_zs_bound(0, 65536) != 0 || qzd_zs_bound(5, 0) != 0) { fprintf(stderr, "bound\n"); fails++; }
    printf("sim_zstd: %d failures\n", fails);
    return fails ? 1 : 0;
}
#endif
