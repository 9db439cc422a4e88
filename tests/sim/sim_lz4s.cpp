/*
 * sim_lz4s.cpp — runs the LZ4s kernel (qatzip_amd/csrc/qzk_lz4s.h) on the CPU SIMT emulator (hipsim.h) behind a C ABI for
 * tests/test_sim_lz4s.py and tests/golden/gen_lz4s.py.  TEST INFRASTRUCTURE, as sim_driver.cpp.
 * The launch sequence is the device layer's (qzd_device.hip, qzd_lz4s_compress_blocks): the pull kernel over all chunks,
 * then scan and gather restated in plain C++ (they are not kernels of a header).
 */
#define QZ_SIM 1
#include "hipsim.h"
#include "../../qatzip_amd/csrc/qzk_lz4s.h"
#include <vector>

extern "C" {

uint32_t sim_lz4s_bound_block(uint32_t c) { return QZK_L4S_BOUND(c); }

/* every block_sz bytes of src a block, by `waves` persistent waves (0: one per chunk).  The slots are filled with 0xEE and
 * have 64 guard bytes behind the bound, which must still be 0xEE afterwards (-3 otherwise).  block_len (optional): per
 * block, its length with the size word.  Returns 0, -1 when out_cap does not hold the result, -2 for bad parameters. */
int sim_lz4s(const uint8_t *src, uint64_t total, uint32_t block_sz, uint32_t mini_match, uint32_t waves,
             uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *block_len)
{
    if (mini_match < 3 || mini_match > 4 || block_sz < QZK_L4S_MINBLK || block_sz > QZK_L4S_MAXBLK || (block_sz & (block_sz - 1))) return -2;
    *out_len = 0;
    if (!total) return 0;
    const uint32_t nb = (uint32_t)((total + block_sz - 1) / block_sz);
    const uint32_t bound = QZK_L4S_BOUND(block_sz), stride = (bound + 64 + 15) & ~15u;
    std::vector<uint8_t> slots((size_t)nb * stride, (uint8_t)0xEE);
    std::vector<uint32_t> lens(nb);
    uint32_t counter = 0;
    if (!waves || waves > nb) waves = nb;
    sim::launch(waves, 64, 0, [&] { qzk_lz4s_pull_kernel(src, total, block_sz, nb, slots.data(), stride, lens.data(), mini_match, &counter); });
    uint64_t running = 0;
    for (uint32_t i = 0; i < nb; i++) {
        const uint64_t off = (uint64_t)i * block_sz;
        const uint32_t n = (uint32_t)(total - off < block_sz ? total - off : block_sz);
        if (lens[i] > QZK_L4S_BOUND(n)) return -3;
        for (uint32_t k = lens[i]; k < stride; k++) if (slots[(size_t)i * stride + k] != 0xEE) return -3;
        if (running + lens[i] > out_cap) return -1;
        memcpy(out + running, slots.data() + (size_t)i * stride, lens[i]);
        running += lens[i];
        if (block_len) block_len[i] = lens[i];
    }
    *out_len = running;
    return 0;
}

}
