/*
 * sim_meta.cpp — runs the kernels of block-addressable compression (qatzip_amd/csrc/qzk_meta.h: programmable CRC, XXH32 of
 * ranges, block plan / pack / unpack) on the CPU SIMT emulator (hipsim.h) behind a C ABI for tests/test_sim_meta.py.
 * TEST INFRASTRUCTURE, as sim_driver.cpp.  Launch shapes are the device layer's (qzd_meta.hip).
 */
#define QZ_SIM 1
#include "hipsim.h"
#include "../../qatzip_amd/csrc/qzk_meta.h"
#include <vector>

extern "C" {

/* ranges: nranges x {u64 off, u32 len, u32 pad}; start: finalised CRCs of what came before, or NULL; out: finalised CRCs */
void sim_crcn(const uint8_t *data, const void *ranges, uint32_t nranges, uint32_t width, uint64_t poly, uint64_t init,
              uint32_t refin, uint32_t refout, uint64_t xorout, const uint64_t *start, uint64_t *out)
{
    const qzk_crcn_cfg cfg = qzk_crcn_make(width, poly, init, refin, refout, xorout);
    sim::launch(nranges, QZK_CRCN_T, 0, [&] { qzk_crcn_kernel(data, (const qzk_mrange *)ranges, nranges, cfg, start, out); });
}

void sim_xxh32_ranges(const uint8_t *data, const void *ranges, uint32_t nranges, uint32_t *out)
{
    sim::launch(nranges, 64, 0, [&] { qzk_xxh32_ranges_kernel(data, (const qzk_mrange *)ranges, nranges, out); });
}

/* plan + pack of nblocks blocks: streams = the slot streams back to back (slot_len each), plain = the n input bytes.
 * pos: nblocks x {u64 offset, u32 size, u32 flags}; in_rng / out_rng: nblocks x range; dst is written up to dst_cap. */
void sim_blocks_pack(const uint8_t *streams, const uint32_t *slot_len, const uint8_t *plain, uint64_t n, uint32_t block_sz,
                     uint32_t nblocks, uint32_t thrshold, uint8_t *dst, uint64_t dst_cap, void *pos, void *in_rng, void *out_rng,
                     uint64_t *total)
{
    std::vector<uint64_t> from(nblocks);
    sim::launch(1, QZK_PLAN_T, 0, [&] {
        qzk_blocks_plan_kernel(slot_len, nblocks, n, block_sz, thrshold, dst_cap, (qzk_blockpos *)pos, from.data(),
                               (qzk_mrange *)in_rng, (qzk_mrange *)out_rng, total);
    });
    sim::launch(nblocks, 256, 0, [&] {
        qzk_blocks_pack_kernel(streams, plain, (const qzk_blockpos *)pos, from.data(), nblocks, dst, dst_cap);
    });
}

/* jobs: njobs x {u64 in_off, u64 out_off, u32 len, u32 pad} */
void sim_blocks_unpack(const uint8_t *comp, uint8_t *out, const void *jobs, uint32_t njobs)
{
    sim::launch(njobs, 256, 0, [&] { qzk_blocks_unpack_kernel(comp, out, (const qzk_copyjob *)jobs, njobs); });
}

}
