/*
 * qzd_zstdd.hip — device layer of the zstd decoder (include/qzamd_device.h, qzd_zstd_decompress_frames): the frames of a
 * call in rounds whose scratch stays under QZD_ZD_SCRATCH_CAP (qzd_zstdd_host.h), per round three launches - stage E,
 * stage X, the content checksums (qzk_zstdd.h) - whatever the number of frames; one wait at the end of the call.
 * Frames whose block count the caller gives (qzd_zstd_decompress_frames_ex, include/qzamd_zstd_blocks.h) and that the route
 * takes (qzd_zstdd_host.h) have their bit streams read a block per lane group instead: five launches of qzk_zstdd_blocks.h in
 * place of stage E for those frames, stage E for the others of the round, then stage X and the checksums over all of them.  A
 * call without such a frame issues the three launches per round and nothing else.
 * Developer aid for tools/zstd_decode_bench.py: QATZIP_AMD_ZSTDD_STAGES=1 launches stage E alone, =3 stages E and X (the
 * answers of such a call mean nothing); the launches are serial on one stream, so the differences are the stages' times.
 */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "qzd_internal.h"
#include "qzk_zstdd.h"
#include "qzk_zstdd_blocks.h"
#include "qzamd_zstd_blocks.h"
#include "qzd_zstdd_host.h"

/* the device-only scratch the compress paths carve their symbols from (calls of one context never overlap) */
static int zd_scratch(qzd_ctx *c, size_t need)
{
    if (need <= c->lane_cap) return QZD_OK;
    hipDeviceSynchronize();
    if (c->d_lane) hipFree(c->d_lane);
    c->d_lane = NULL; c->lane_cap = 0;
    need = (need + 65535) & ~(size_t)65535;
    if (hipMalloc((void **)&c->d_lane, need) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(c->err, sizeof(c->err), "zstd decode: %zu bytes of scratch could not be had", need);
        return QZD_ERR_NOMEM;
    }
    c->lane_cap = need;
    return QZD_OK;
}

extern "C" int qzd_zstd_decode_route(qzd_ctx *c, int route)
{
    if (!c || route < 0 || route > 2) return QZD_ERR_PARAM;
    c->zstdd_route = route;
    return QZD_OK;
}

extern "C" int qzd_zstd_decompress_frames_ex(qzd_ctx *c, const uint8_t *d_comp, uint8_t *d_out, const void *h_segs,
                                             uint32_t nsegs, void *h_res, const uint32_t *h_nblocks)
{
    if (!c || !h_segs || !h_res) return QZD_ERR_PARAM;
    if (nsegs == 0) return QZD_OK;
    if (!d_comp || !d_out) return QZD_ERR_PARAM;
    hipSetDevice(c->device);
    static_assert(sizeof(qzk_zdseg) == sizeof(qzd_lz4seg) && sizeof(qzk_zdres) == sizeof(qzd_lz4res), "the segment records of the LZ4 decoder");
    const qzk_zdseg *hs = (const qzk_zdseg *)h_segs;
    if (c->zstdd_route == 1) h_nblocks = NULL;
    bool any = false;
    for (uint32_t i = 0; h_nblocks && i < nsegs && !any; i++) any = qzd_zdb_routed(c->zstdd_route, h_nblocks[i]);
    if (!any) h_nblocks = NULL;
    const size_t sb = ((size_t)nsegs * sizeof(qzk_zdseg) + 15) & ~(size_t)15, rb = ((size_t)nsegs * sizeof(qzk_zdres) + 15) & ~(size_t)15,
                 pb = ((size_t)nsegs * sizeof(qzk_zdplan) + 15) & ~(size_t)15;
    /* with routed frames: stage E's copy of the segments (a routed frame has no input there) and the routed frames */
    const size_t fb = h_nblocks ? ((size_t)nsegs * sizeof(qzk_zdb_frame) + 15) & ~(size_t)15 : 0;
    int rc = qzd_aux_reserve(c, sb + rb + pb + (h_nblocks ? sb + fb : 0) + 64);
    if (rc) return rc;
    qzk_zdseg *d_segs = (qzk_zdseg *)c->d_aux;
    qzk_zdres *d_res = (qzk_zdres *)(c->d_aux + sb);
    qzk_zdplan *d_plan = (qzk_zdplan *)(c->d_aux + sb + rb), *h_plan = (qzk_zdplan *)(c->h_aux + sb + rb);
    qzk_zdseg *d_esegs = (qzk_zdseg *)(c->d_aux + sb + rb + pb), *h_esegs = (qzk_zdseg *)(c->h_aux + sb + rb + pb);
    qzk_zdb_frame *d_fr = (qzk_zdb_frame *)(c->d_aux + sb + rb + pb + sb), *h_fr = (qzk_zdb_frame *)(c->h_aux + sb + rb + pb + sb);
    /* the rounds, and the largest one's scratch: the descriptors of its routed frames behind its literals and records */
    struct Round { uint32_t k, nfr; uint64_t nblk, desc_off; };
    uint64_t most = 0;
    std::vector<Round> rounds;
    uint32_t nfr_all = 0;
    for (uint32_t first = 0; first < nsegs; first += rounds.back().k) {
        uint64_t bytes = 0;
        Round r;
        r.k = qzd_zd_round(hs, first, nsegs, QZD_ZD_SCRATCH_CAP, h_plan + first, &bytes);
        r.nfr = 0; r.nblk = 0; r.desc_off = (bytes + 15) & ~15ull;
        if (h_nblocks) {
            r.nfr = qzd_zdb_round(hs, h_nblocks, first, r.k, c->zstdd_route, h_fr + nfr_all, &r.nblk);
            if (r.nblk > 0x7fffffffull) { snprintf(c->err, sizeof(c->err), "zstd decode: %llu blocks in one round", (unsigned long long)r.nblk); return QZD_ERR_PARAM; }
            if (r.nfr) bytes = r.desc_off + qzd_zdb_desc_bytes(r.nblk);
            nfr_all += r.nfr;
        }
        rounds.push_back(r);
        if (bytes > most) most = bytes;
    }
    rc = zd_scratch(c, (size_t)most);
    if (rc) return rc;
    hipStream_t st = c->st[0];
    memcpy(c->h_aux, hs, (size_t)nsegs * sizeof(qzk_zdseg));
    HIPCHK(c, hipMemcpyAsync(d_segs, c->h_aux, (size_t)nsegs * sizeof(qzk_zdseg), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_plan, h_plan, (size_t)nsegs * sizeof(qzk_zdplan), hipMemcpyHostToDevice, st));
    if (nfr_all) {
        memcpy(h_esegs, hs, (size_t)nsegs * sizeof(qzk_zdseg));
        uint32_t first = 0, f0 = 0;
        for (const Round &r : rounds) {
            for (uint32_t j = 0; j < r.nfr; j++) h_esegs[first + h_fr[f0 + j].seg].in_len = 0;
            first += r.k; f0 += r.nfr;
        }
        HIPCHK(c, hipMemcpyAsync(d_esegs, h_esegs, (size_t)nsegs * sizeof(qzk_zdseg), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_fr, h_fr, (size_t)nfr_all * sizeof(qzk_zdb_frame), hipMemcpyHostToDevice, st));
    }
    HIPCHK(c, hipEventRecord(c->ev_begin, st));
    const char *sv = getenv("QATZIP_AMD_ZSTDD_STAGES");
    const int stages = sv && sv[0] ? atoi(sv) | 1 : 7;
    uint32_t first = 0, f0 = 0;
    for (const Round &r : rounds) {
        const uint32_t k = r.k;
        if (r.nfr < k)
            hipLaunchKernelGGL(qzk_zstdd_entropy_kernel, dim3((k + QZK_ZD_G - 1) / QZK_ZD_G), dim3(64), 0, st, d_comp, (r.nfr ? d_esegs : d_segs) + first,
                               d_plan + first, d_res + first, k, c->d_lane);
        if (r.nfr) {
            qzk_zdb_desc *d_desc = (qzk_zdb_desc *)(c->d_lane + r.desc_off);
            const uint32_t nb = (uint32_t)r.nblk;
            hipLaunchKernelGGL(qzk_zstdd_bplan_kernel, dim3(r.nfr), dim3(64), 0, st, d_comp, d_segs + first, d_plan + first, d_fr + f0, r.nfr, d_desc,
                               (uint32_t *)NULL);
            hipLaunchKernelGGL(qzk_zstdd_bentropy_kernel, dim3((nb + QZK_ZD_G - 1) / QZK_ZD_G), dim3(64), 0, st, d_comp, d_segs + first, d_plan + first,
                               d_fr + f0, r.nfr, nb, d_desc, c->d_lane);
            hipLaunchKernelGGL(qzk_zstdd_bscan_kernel, dim3(r.nfr), dim3(64), 0, st, d_fr + f0, r.nfr, d_desc);
            hipLaunchKernelGGL(qzk_zstdd_bfix_kernel, dim3(nb), dim3(64), 0, st, d_segs + first, d_plan + first, d_fr + f0, r.nfr, nb, d_desc, c->d_lane);
            hipLaunchKernelGGL(qzk_zstdd_bfinish_kernel, dim3(r.nfr), dim3(64), 0, st, d_segs + first, d_fr + f0, r.nfr, d_desc, d_res + first);
        }
        if (stages & 2) hipLaunchKernelGGL(qzk_zstdd_exec_kernel, dim3(k), dim3(64), 0, st, d_out, d_segs + first, d_plan + first, d_res + first, k,
                           (const uint8_t *)c->d_lane);
        if (stages & 4) hipLaunchKernelGGL(qzk_zstdd_xxh_kernel, dim3(k), dim3(64), 0, st, d_comp, (const uint8_t *)d_out, d_segs + first, d_res + first, k);
        first += k; f0 += r.nfr;
    }
    HIPCHK(c, hipEventRecord(c->ev_end, st));
    HIPCHK(c, hipMemcpyAsync(h_res, d_res, (size_t)nsegs * sizeof(qzk_zdres), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    for (uint32_t i = 0; i < nsegs; i++) ((qzk_zdres *)h_res)[i].pad = 0;    /* (stage E's record count) */
    return QZD_OK;
}

extern "C" int qzd_zstd_decompress_frames(qzd_ctx *c, const uint8_t *d_comp, uint8_t *d_out, const void *h_segs,
                                          uint32_t nsegs, void *h_res)
{
    return qzd_zstd_decompress_frames_ex(c, d_comp, d_out, h_segs, nsegs, h_res, NULL);
}

/* the Plan walk without descriptors, a wave per frame, and one readback */
extern "C" int qzd_zstd_count_blocks(qzd_ctx *c, const uint8_t *d_comp, const void *h_segs, uint32_t nsegs, uint32_t *h_nblocks)
{
    if (!c || !h_segs || !h_nblocks) return QZD_ERR_PARAM;
    if (nsegs == 0) return QZD_OK;
    if (!d_comp) return QZD_ERR_PARAM;
    hipSetDevice(c->device);
    const qzk_zdseg *hs = (const qzk_zdseg *)h_segs;
    const size_t sb = ((size_t)nsegs * sizeof(qzk_zdseg) + 15) & ~(size_t)15, fb = ((size_t)nsegs * sizeof(qzk_zdb_frame) + 15) & ~(size_t)15,
                 cb = (size_t)nsegs * sizeof(uint32_t);
    int rc = qzd_aux_reserve(c, sb + fb + cb + 64);
    if (rc) return rc;
    qzk_zdseg *d_segs = (qzk_zdseg *)c->d_aux;
    qzk_zdb_frame *d_fr = (qzk_zdb_frame *)(c->d_aux + sb), *h_fr = (qzk_zdb_frame *)(c->h_aux + sb);
    uint32_t *d_cnt = (uint32_t *)(c->d_aux + sb + fb);
    memcpy(c->h_aux, hs, (size_t)nsegs * sizeof(qzk_zdseg));
    memset(h_fr, 0, (size_t)nsegs * sizeof(qzk_zdb_frame));
    for (uint32_t i = 0; i < nsegs; i++) { h_fr[i].seg = i; h_fr[i].hint = 0xffffffffu; }
    hipStream_t st = c->st[0];
    HIPCHK(c, hipMemcpyAsync(d_segs, c->h_aux, (size_t)nsegs * sizeof(qzk_zdseg), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_fr, h_fr, (size_t)nsegs * sizeof(qzk_zdb_frame), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(qzk_zstdd_bplan_kernel, dim3(nsegs), dim3(64), 0, st, d_comp, d_segs, (const qzk_zdplan *)NULL, d_fr, nsegs, (qzk_zdb_desc *)NULL, d_cnt);
    HIPCHK(c, hipMemcpyAsync(h_nblocks, d_cnt, cb, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return QZD_OK;
}
