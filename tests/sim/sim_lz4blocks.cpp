/*
 * sim_lz4blocks.cpp — runs the LZ4 frame decoders (qatzip_amd/csrc/qzk_lz4.h: qzk_lz4d_kernel and the plan / size / scan /
 * block / finish kernels of K5b) on the CPU SIMT emulator (hipsim.h) behind a C ABI for tests/test_sim_lz4_blocks.py.
 * TEST INFRASTRUCTURE, as sim_driver.cpp.
 * The launch sequence and the routing are the device layer's (qzd_device.hip, qzd_lz4_decompress_frames), restated in
 * plain C++: candidates by length, the plan's verdicts, the frames it leaves to the one-wave kernel in one launch with the
 * small ones, the block kernels for the rest.
 */
#define QZ_SIM 1
#include "hipsim.h"
#include "../../qatzip_amd/csrc/qzk_lz4.h"
#include <vector>

extern "C" {

/* route: 0 auto, 1 every frame on one wave, 2 blocks wherever a frame qualifies (minblk = 2 for both 0 and 2, as the device
 * layer has it).  block_waves (optional): waves of the block launches - 0 when no frame went that way */
int sim_lz4_frames(const uint8_t *comp, uint8_t *out, const qzk_lz4seg *segs, uint32_t nsegs, int route, qzk_lz4res *res,
                   uint32_t *block_waves)
{
    if (block_waves) *block_waves = 0;
    if (nsegs == 0) return 0;
    std::vector<qzk_lz4cand> cand;
    uint32_t first = 0;
    if (route != 1) for (uint32_t i = 0; i < nsegs; i++) if (segs[i].in_len > QZK_LZ4_CAND) {
        qzk_lz4cand cd; cd.seg = i; cd.first = first; cd.cap = QZK_LZ4_SHARE(segs[i].in_len); cd.pad = 0;
        cand.push_back(cd); first += cd.cap;
    }
    const uint32_t ncand = (uint32_t)cand.size();
    if (ncand == 0) {
        sim::launch(nsegs, 64, 0, [&] { qzk_lz4d_kernel(comp, out, segs, res, nsegs); });
        return 0;
    }
    std::vector<qzk_lz4blk> table(first);
    std::vector<uint32_t> dlen(first, 0xABCDABCDu), ooff(first, 0xABCDABCDu);
    std::vector<qzk_lz4plan> plan(ncand);
    sim::launch(ncand, 64, 0, [&] { qzk_lz4d_plan_kernel(comp, segs, cand.data(), ncand, 2u, table.data(), plan.data(), res); });
    std::vector<qzk_lz4fr> fr;
    std::vector<qzk_lz4seg> segs2;
    std::vector<uint32_t> idx2;
    uint32_t nw = 0, k = 0;
    for (uint32_t i = 0; i < nsegs; i++) {
        if (segs[i].in_len > QZK_LZ4_CAND) {
            const qzk_lz4plan pl = plan[k]; const qzk_lz4cand cd = cand[k]; k++;
            if (pl.route == QZK_LZ4P_DONE) continue;
            if (pl.route == QZK_LZ4P_BLOCKS) {
                qzk_lz4fr F; F.seg = i; F.first = cd.first; F.nblk = pl.nblk; F.wbase = nw; F.end = pl.end; F.flags = pl.flags; F.status = 0; F.total = 0;
                fr.push_back(F); nw += pl.nblk;
                continue;
            }
        }
        segs2.push_back(segs[i]); idx2.push_back(i);
    }
    const uint32_t nfr = (uint32_t)fr.size(), n2 = (uint32_t)segs2.size();
    std::vector<qzk_lz4res> res2(n2);
    if (n2) sim::launch(n2, 64, 0, [&] { qzk_lz4d_kernel(comp, out, segs2.data(), res2.data(), n2); });
    if (nfr) {
        sim::launch(nw, 64, 0, [&] { qzk_lz4d_size_kernel(comp, segs, table.data(), fr.data(), nfr, nw, dlen.data()); });
        sim::launch(nfr, 64, 0, [&] { qzk_lz4d_scan_kernel(segs, fr.data(), nfr, dlen.data(), ooff.data()); });
        sim::launch(nw, 64, 0, [&] { qzk_lz4d_block_kernel(comp, out, segs, table.data(), fr.data(), nfr, nw, dlen.data(), ooff.data()); });
        sim::launch(nfr, 64, 0, [&] { qzk_lz4d_finish_kernel(comp, out, segs, fr.data(), nfr, res); });
    }
    for (uint32_t j = 0; j < n2; j++) res[idx2[j]] = res2[j];
    if (block_waves) *block_waves = nw;
    return 0;
}

}
