/*
 * sim_lz4hc.cpp — runs the LZ4-HC kernels (qatzip_amd/csrc/qzk_lz4hc.h) on the CPU SIMT emulator (hipsim.h) behind a C ABI
 * for tests/test_sim_lz4hc.py and tools/sim_fuzz_lz4hc.py.  TEST INFRASTRUCTURE, as sim_driver.cpp.
 * The launch sequence is the device layer's (qzd_device.hip, lz4hc_impl): content hashes, per round chains, parse, scan,
 * gather, then finish - scan and gather restated in plain C++ (they are not kernels of a header).
 */
#define QZ_SIM 1
#include "hipsim.h"
#include "../../qatzip_amd/csrc/qzk_lz4hc.h"
#include <vector>

static uint32_t hc_stride() { return (QZK_LZ4_MAXBLK + QZK_HC_HDRMAX + 4 + 8 + 15) & ~15u; }

extern "C" {

/* the frames of one call: every frame_sz bytes a frame (frame_sz >= total: one frame), in rounds of `batch` blocks.
 * block_len (optional): per block, what its slot held.  Returns 0, -1 when out_cap does not hold the result. */
int sim_lz4hc(const uint8_t *src, uint64_t total, uint32_t frame_sz, int level, uint32_t hw_hdr, uint32_t batch,
              uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *block_len)
{
    const int attempts = qzk_hc_attempts(level);
    if (!attempts || !frame_sz) return -2;
    const uint32_t bpf = (frame_sz + QZK_LZ4_MAXBLK - 1) / QZK_LZ4_MAXBLK;
    const uint32_t nfr = total ? (uint32_t)((total + frame_sz - 1) / frame_sz) : 1;
    const uint64_t lastlen = total - (uint64_t)(nfr - 1) * frame_sz;
    const uint32_t nb = (nfr - 1) * bpf + (lastlen ? (uint32_t)((lastlen + QZK_LZ4_MAXBLK - 1) / QZK_LZ4_MAXBLK) : 1);
    if (!batch || batch > nb) batch = nb;
    const uint32_t stride = hc_stride();
    std::vector<uint32_t> head((size_t)batch * QZK_HC_HSIZE), lens(nb), xx(nfr);
    std::vector<uint16_t> chain((size_t)batch * QZK_HC_WIN, (uint16_t)0xABCD);
    std::vector<uint8_t> slots((size_t)batch * stride, (uint8_t)0xEE);
    std::vector<uint64_t> offs(nb);
    uint64_t running = 0;
    sim::launch(nfr, 64, 0, [&] { qzk_lz4hc_xxh_kernel(src, total, frame_sz, nfr, xx.data()); });
    for (uint32_t g0 = 0; g0 < nb; g0 += batch) {
        const uint32_t bn = nb - g0 < batch ? nb - g0 : batch;
        std::fill(head.begin(), head.end(), 0u);
        sim::launch(bn, 64, 0, [&] { qzk_lz4hc_chain_kernel(src, total, frame_sz, bpf, g0, bn, head.data(), chain.data()); });
        sim::launch(bn, 64, 0, [&] { qzk_lz4hc_parse_kernel(src, total, frame_sz, bpf, g0, bn, chain.data(), slots.data(), stride, lens.data() + g0, hw_hdr, attempts); });
        for (uint32_t i = 0; i < bn; i++) { offs[g0 + i] = running; running += lens[g0 + i]; }
        if (running > out_cap) return -1;
        for (uint32_t i = 0; i < bn; i++) memcpy(out + offs[g0 + i], slots.data() + (size_t)i * stride, lens[g0 + i]);
    }
    if (block_len) for (uint32_t i = 0; i < nb; i++) block_len[i] = lens[i];
    sim::launch((nfr + 63) / 64, 64, 0, [&] { qzk_lz4hc_finish_kernel(total, frame_sz, bpf, 0, nb, nb, offs.data(), lens.data(), xx.data(), out, out_cap); });
    *out_len = running;
    return 0;
}

/* block g of the call ALONE: its chains and its parse, nothing of the blocks around it but their bytes.  slot gets what
 * the block's slot holds ([header][block word][block][8 free bytes]); returns its length */
uint32_t sim_lz4hc_block(const uint8_t *src, uint64_t total, uint32_t frame_sz, int level, uint32_t g, uint8_t *slot)
{
    const int attempts = qzk_hc_attempts(level);
    const uint32_t bpf = (frame_sz + QZK_LZ4_MAXBLK - 1) / QZK_LZ4_MAXBLK;
    std::vector<uint32_t> head(QZK_HC_HSIZE, 0u);
    std::vector<uint16_t> chain(QZK_HC_WIN, (uint16_t)0xABCD);
    uint32_t len = 0;
    sim::launch(1, 64, 0, [&] { qzk_lz4hc_chain_kernel(src, total, frame_sz, bpf, g, 1, head.data(), chain.data()); });
    sim::launch(1, 64, 0, [&] { qzk_lz4hc_parse_kernel(src, total, frame_sz, bpf, g, 1, chain.data(), slot, hc_stride(), &len, 0, attempts); });
    return len;
}

uint32_t sim_lz4hc_stride(void) { return hc_stride(); }

}

#ifdef SIM_LZ4HC_MAIN
/* A program of its own for the sanitizers (tests/test_sim_lz4hc_traps.py builds it with -fsanitize=address,undefined):
 * reads inputs (u32le length + bytes, one after the other) from the file named on its command line, puts each into a heap
 * buffer of EXACTLY its length and runs level 3 in rounds of one block and level 8 in one round on it.  A search, a count or
 * a chain trip that reads past an input's end stops it: that is what this program is for.  Of the bytes it checks only that
 * a frame came out; the comparison with liblz4's pinned bytes is the test's. */
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned count = 0, failures = 0;
    uint8_t lenb[4];
    while (fread(lenb, 1, 4, f) == 4) {
        const uint32_t n = lenb[0] | lenb[1] << 8 | lenb[2] << 16 | (uint32_t)lenb[3] << 24;
        uint8_t *src = (uint8_t *)malloc(n ? n : 1);
        if (n && fread(src, 1, n, f) != n) return 2;
        const uint64_t cap = (uint64_t)n + 64 + 32 * (n / QZK_LZ4_MAXBLK + 3);
        for (int level = 3; level <= 8; level += 5) {
            uint8_t *a = (uint8_t *)malloc(cap);
            uint64_t la = 0;
            const int ra = sim_lz4hc(src, n, n ? n : 1, level, 0, level == 3 ? 1 : 0, a, cap, &la, NULL);
            if (ra || la < 11 || la > cap) { failures++; printf("input %u (n = %u) level %d: %d, %llu bytes\n", count, n, level, ra, (unsigned long long)la); }
            free(a);
        }
        free(src);
        count++;
    }
    fclose(f);
    printf("%u inputs, %u failures\n", count, failures);
    return failures ? 1 : 0;
}
#endif
