/*
 * qzd_zstdd.hip — device layer of the zstd decoder (include/qzamd_device.h, qzd_zstd_decompress_frames): the frames of a
 * call in rounds whose scratch stays under QZD_ZD_SCRATCH_CAP (qzd_zstdd_host.h), per round three launches - stage E,
 * stage X, the content checksums (qzk_zstdd.h) - whatever the number of frames; one wait at the end of the call.
 * Developer aid for tools/zstd_decode_bench.py: QATZIP_AMD_ZSTDD_STAGES=1 launches stage E alone, =3 stages E and X (the
 * answers of such a call mean nothing); the launches are serial on one stream, so the differences are the stages' times.
 */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "qzd_internal.h"
#include "qzk_zstdd.h"
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

extern "C" int qzd_zstd_decompress_frames(qzd_ctx *c, const uint8_t *d_comp, uint8_t *d_out, const void *h_segs,
                                          uint32_t nsegs, void *h_res)
{
    if (!c || !h_segs || !h_res) return QZD_ERR_PARAM;
    if (nsegs == 0) return QZD_OK;
    if (!d_comp || !d_out) return QZD_ERR_PARAM;
    hipSetDevice(c->device);
    static_assert(sizeof(qzk_zdseg) == sizeof(qzd_lz4seg) && sizeof(qzk_zdres) == sizeof(qzd_lz4res), "the segment records of the LZ4 decoder");
    const qzk_zdseg *hs = (const qzk_zdseg *)h_segs;
    const size_t sb = ((size_t)nsegs * sizeof(qzk_zdseg) + 15) & ~(size_t)15, rb = ((size_t)nsegs * sizeof(qzk_zdres) + 15) & ~(size_t)15,
                 pb = (size_t)nsegs * sizeof(qzk_zdplan);
    int rc = qzd_aux_reserve(c, sb + rb + pb + 64);
    if (rc) return rc;
    qzk_zdseg *d_segs = (qzk_zdseg *)c->d_aux;
    qzk_zdres *d_res = (qzk_zdres *)(c->d_aux + sb);
    qzk_zdplan *d_plan = (qzk_zdplan *)(c->d_aux + sb + rb), *h_plan = (qzk_zdplan *)(c->h_aux + sb + rb);
    /* the rounds, and the largest one's scratch */
    uint64_t most = 0;
    std::vector<uint32_t> rounds;
    for (uint32_t first = 0; first < nsegs; first += rounds.back()) {
        uint64_t bytes = 0;
        rounds.push_back(qzd_zd_round(hs, first, nsegs, QZD_ZD_SCRATCH_CAP, h_plan + first, &bytes));
        if (bytes > most) most = bytes;
    }
    rc = zd_scratch(c, (size_t)most);
    if (rc) return rc;
    hipStream_t st = c->st[0];
    memcpy(c->h_aux, hs, (size_t)nsegs * sizeof(qzk_zdseg));
    HIPCHK(c, hipMemcpyAsync(d_segs, c->h_aux, (size_t)nsegs * sizeof(qzk_zdseg), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_plan, h_plan, pb, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(c->ev_begin, st));
    const char *sv = getenv("QATZIP_AMD_ZSTDD_STAGES");
    const int stages = sv && sv[0] ? atoi(sv) | 1 : 7;
    uint32_t first = 0;
    for (const uint32_t k : rounds) {
        hipLaunchKernelGGL(qzk_zstdd_entropy_kernel, dim3((k + QZK_ZD_G - 1) / QZK_ZD_G), dim3(64), 0, st, d_comp, d_segs + first, d_plan + first,
                           d_res + first, k, c->d_lane);
        if (stages & 2) hipLaunchKernelGGL(qzk_zstdd_exec_kernel, dim3(k), dim3(64), 0, st, d_out, d_segs + first, d_plan + first, d_res + first, k,
                           (const uint8_t *)c->d_lane);
        if (stages & 4) hipLaunchKernelGGL(qzk_zstdd_xxh_kernel, dim3(k), dim3(64), 0, st, d_comp, (const uint8_t *)d_out, d_segs + first, d_res + first, k);
        first += k;
    }
    HIPCHK(c, hipEventRecord(c->ev_end, st));
    HIPCHK(c, hipMemcpyAsync(h_res, d_res, (size_t)nsegs * sizeof(qzk_zdres), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    for (uint32_t i = 0; i < nsegs; i++) ((qzk_zdres *)h_res)[i].pad = 0;    /* (stage E's record count) */
    return QZD_OK;
}
