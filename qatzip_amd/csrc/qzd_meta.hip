/*
 * qzd_meta.hip — device layer of block-addressable compression (include/qzamd_device.h, "block-addressable compression"):
 * CRCs under a caller's polynomial, XXH32 of ranges, and a buffer as independent blocks with a table beside the data.
 * Kernels: qzk_meta.h (K10-K12).  The deflate and inflate work is the existing one: qzd_deflate_slots writes every block
 * as a raw-deflate stream of its own, qzd_inflate_segments decodes the compressed blocks of a table.
 *
 * Launches of a compress call, whatever the number of blocks: what qzd_deflate_slots takes, then plan (1), pack (1),
 * XXH32 (1) and CRC (4: plaintext and destination, 32 and 64 bits).  A decompress call: what qzd_inflate_segments takes,
 * unpack (1, when there are stored blocks), XXH32 (1).
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>

#include "qzd_internal.h"
#include "qz_frame.h"
#include "qzk_meta.h"

static const qzd_crccfg k_crc32_gzip = {0x04C11DB7ull, 0xFFFFFFFFull, 1, 1, 0xFFFFFFFFull};
static const qzd_crccfg k_crc64_ecma = {0x42F0E1EBA9EA3693ull, 0, 0, 0, 0};

static int meta_reserve(qzd_ctx *c, size_t need)
{
    if (need <= c->meta_cap) return QZD_OK;
    hipDeviceSynchronize();
    if (c->d_meta) hipFree(c->d_meta);
    c->d_meta = NULL; c->meta_cap = 0;
    need = (need + 65535) & ~(size_t)65535;
    if (hipMalloc((void **)&c->d_meta, need) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(c->err, sizeof(c->err), "no device memory for %zu bytes of block scratch", need);
        return QZD_ERR_NOMEM;
    }
    c->meta_cap = need;
    return QZD_OK;
}

static bool cfg_ok(int width, const qzd_crccfg *g)
{
    if (width != 32 && width != 64) return false;
    if (g->reflect_in > 1 || g->reflect_out > 1 || !(g->polynomial & 1)) return false;
    if (width == 32 && ((g->polynomial | g->initial_value | g->xor_out) >> 32)) return false;
    return true;
}
static qzk_crcn_cfg kcfg(int width, const qzd_crccfg *g)
{ return qzk_crcn_make((uint32_t)width, g->polynomial, g->initial_value, g->reflect_in, g->reflect_out, g->xor_out); }

/* carve `bytes` out of a scratch area in pieces of 256 */
static uint8_t *carve(uint8_t **p, size_t bytes) { uint8_t *r = *p; *p += (bytes + 255) & ~(size_t)255; return r; }
static size_t carved(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

extern "C" int qzd_crcn_ranges(qzd_ctx *c, const uint8_t *d_data, const void *h_ranges, uint32_t nranges, int width,
                               const qzd_crccfg *cfg, const uint64_t *h_start, uint64_t *h_out)
{
    if (!c || !h_ranges || !h_out || !cfg || !cfg_ok(width, cfg)) return QZD_ERR_PARAM;
    if (nranges == 0) return QZD_OK;
    hipSetDevice(c->device);
    const size_t rb = (size_t)nranges * sizeof(qzk_mrange), vb = (size_t)nranges * 8;
    int rc = meta_reserve(c, carved(rb) + 2 * carved(vb));
    if (rc) return rc;
    uint8_t *p = c->d_meta;
    qzk_mrange *d_r = (qzk_mrange *)carve(&p, rb);
    uint64_t *d_s = (uint64_t *)carve(&p, vb), *d_o = (uint64_t *)carve(&p, vb);
    hipStream_t st = c->st[0];
    HIPCHK(c, hipMemcpyAsync(d_r, h_ranges, rb, hipMemcpyHostToDevice, st));
    if (h_start) HIPCHK(c, hipMemcpyAsync(d_s, h_start, vb, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(qzk_crcn_kernel, dim3(nranges), dim3(QZK_CRCN_T), 0, st, d_data, d_r, nranges, kcfg(width, cfg),
                       h_start ? (const uint64_t *)d_s : (const uint64_t *)NULL, d_o);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out, d_o, vb, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return QZD_OK;
}

extern "C" int qzd_xxh32_ranges(qzd_ctx *c, const uint8_t *d_data, const void *h_ranges, uint32_t nranges, uint32_t *h_hash)
{
    if (!c || !h_ranges || !h_hash) return QZD_ERR_PARAM;
    if (nranges == 0) return QZD_OK;
    hipSetDevice(c->device);
    const size_t rb = (size_t)nranges * sizeof(qzk_mrange), vb = (size_t)nranges * 4;
    int rc = meta_reserve(c, carved(rb) + carved(vb));
    if (rc) return rc;
    uint8_t *p = c->d_meta;
    qzk_mrange *d_r = (qzk_mrange *)carve(&p, rb);
    uint32_t *d_h = (uint32_t *)carve(&p, vb);
    hipStream_t st = c->st[0];
    HIPCHK(c, hipMemcpyAsync(d_r, h_ranges, rb, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(qzk_xxh32_ranges_kernel, dim3(nranges), dim3(64), 0, st, d_data, d_r, nranges, d_h);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_hash, d_h, vb, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return QZD_OK;
}

extern "C" int qzd_blocks_compress(qzd_ctx *c, const uint8_t *d_src, uint64_t n, uint32_t block_sz, int level, uint32_t thrshold,
                                   const qzd_crccfg *cfg32, const qzd_crccfg *cfg64, uint8_t *d_dst, uint64_t dst_cap,
                                   qzd_blockrec *h_records, uint64_t *h_out_len)
{
    if (!c || !h_out_len) return QZD_ERR_PARAM;
    *h_out_len = 0;
    if (n == 0) return QZD_OK;
    if (!d_src || !d_dst || !h_records || block_sz == 0 || block_sz > 512u * 1024u || level < 1 || level > 9) return QZD_ERR_PARAM;
    if (!cfg32) cfg32 = &k_crc32_gzip;
    if (!cfg64) cfg64 = &k_crc64_ecma;
    if (!cfg_ok(32, cfg32) || !cfg_ok(64, cfg64)) return QZD_ERR_PARAM;
    const uint64_t nb64 = (n + block_sz - 1) / block_sz;
    if (nb64 > 0x7fffffffull / 64) return QZD_ERR_PARAM;
    const uint32_t nb = (uint32_t)nb64;
    hipSetDevice(c->device);
    /* scratch: the slot streams back to back (worst case: stored deflate blocks), the plan, the ranges, hash and CRCs */
    const uint64_t worst = qz_deflate_bound(n, nb, block_sz);
    const size_t need = carved(worst + 64) + carved((size_t)nb * sizeof(qzk_blockpos)) + carved((size_t)nb * 8) +
                        2 * carved((size_t)nb * sizeof(qzk_mrange)) + carved((size_t)nb * 4) + 4 * carved((size_t)nb * 8) + 256;
    int rc = meta_reserve(c, need);
    if (rc) return rc;
    uint8_t *p = c->d_meta;
    uint8_t *d_streams = carve(&p, worst + 64);
    qzk_blockpos *d_pos = (qzk_blockpos *)carve(&p, (size_t)nb * sizeof(qzk_blockpos));
    uint64_t *d_from = (uint64_t *)carve(&p, (size_t)nb * 8);
    qzk_mrange *d_in = (qzk_mrange *)carve(&p, (size_t)nb * sizeof(qzk_mrange));
    qzk_mrange *d_outr = (qzk_mrange *)carve(&p, (size_t)nb * sizeof(qzk_mrange));
    uint32_t *d_hash = (uint32_t *)carve(&p, (size_t)nb * 4);
    uint64_t *d_crc[4];
    for (int i = 0; i < 4; i++) d_crc[i] = (uint64_t *)carve(&p, (size_t)nb * 8);
    uint64_t *d_total = (uint64_t *)carve(&p, 8);

    std::vector<uint32_t> cdesc(nb);
    for (uint32_t k = 0; k < nb; k++) {
        const uint64_t left = n - (uint64_t)k * block_sz;
        cdesc[k] = (uint32_t)(left < block_sz ? left : block_sz) | 0x80000000u;       /* every block closes its stream */
    }
    uint64_t produced = 0;
    rc = qzd_deflate_slots(c, d_src, nb, block_sz, level, cdesc.data(), d_streams, worst, &produced, NULL, NULL);
    if (rc) return rc;
    /* c->d_len now holds every slot's stream length (what qzd_chunk_lens reads) */
    hipStream_t st = c->st[0];
    hipLaunchKernelGGL(qzk_blocks_plan_kernel, dim3(1), dim3(QZK_PLAN_T), 0, st, (const uint32_t *)c->d_len, nb, n, block_sz,
                       thrshold, dst_cap, d_pos, d_from, d_in, d_outr, d_total);
    hipLaunchKernelGGL(qzk_blocks_pack_kernel, dim3(nb), dim3(256), 0, st, (const uint8_t *)d_streams, d_src,
                       (const qzk_blockpos *)d_pos, (const uint64_t *)d_from, nb, d_dst, dst_cap);
    hipLaunchKernelGGL(qzk_xxh32_ranges_kernel, dim3(nb), dim3(64), 0, st, d_src, (const qzk_mrange *)d_in, nb, d_hash);
    const qzk_crcn_cfg k32 = kcfg(32, cfg32), k64 = kcfg(64, cfg64);
    hipLaunchKernelGGL(qzk_crcn_kernel, dim3(nb), dim3(QZK_CRCN_T), 0, st, d_src, (const qzk_mrange *)d_in, nb, k32, (const uint64_t *)NULL, d_crc[0]);
    hipLaunchKernelGGL(qzk_crcn_kernel, dim3(nb), dim3(QZK_CRCN_T), 0, st, (const uint8_t *)d_dst, (const qzk_mrange *)d_outr, nb, k32, (const uint64_t *)NULL, d_crc[1]);
    hipLaunchKernelGGL(qzk_crcn_kernel, dim3(nb), dim3(QZK_CRCN_T), 0, st, d_src, (const qzk_mrange *)d_in, nb, k64, (const uint64_t *)NULL, d_crc[2]);
    hipLaunchKernelGGL(qzk_crcn_kernel, dim3(nb), dim3(QZK_CRCN_T), 0, st, (const uint8_t *)d_dst, (const qzk_mrange *)d_outr, nb, k64, (const uint64_t *)NULL, d_crc[3]);
    HIPCHK(c, hipGetLastError());
    std::vector<qzk_blockpos> pos(nb);
    std::vector<uint32_t> hash(nb);
    std::vector<uint64_t> crc[4];
    uint64_t total = 0;
    HIPCHK(c, hipMemcpyAsync(pos.data(), d_pos, (size_t)nb * sizeof(qzk_blockpos), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hash.data(), d_hash, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    for (int i = 0; i < 4; i++) { crc[i].resize(nb); HIPCHK(c, hipMemcpyAsync(crc[i].data(), d_crc[i], (size_t)nb * 8, hipMemcpyDeviceToHost, st)); }
    HIPCHK(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    uint64_t written = 0;
    for (uint32_t k = 0; k < nb; k++) {
        qzd_blockrec &r = h_records[k];
        r.offset = pos[k].offset; r.size = pos[k].size; r.flags = pos[k].flags; r.hash = hash[k]; r.pad = 0;
        r.in_crc32 = (uint32_t)crc[0][k]; r.out_crc32 = (uint32_t)crc[1][k]; r.in_crc64 = crc[2][k]; r.out_crc64 = crc[3][k];
        if (r.offset + r.size <= dst_cap) written = r.offset + r.size;
    }
    *h_out_len = written;
    if (total > dst_cap) { snprintf(c->err, sizeof(c->err), "destination too small"); return QZD_ERR_DSTCAP; }
    return QZD_OK;
}

extern "C" int qzd_blocks_decompress(qzd_ctx *c, const uint8_t *d_comp, uint64_t comp_len, const qzd_blockrec *h_records,
                                     uint32_t nblocks, uint32_t block_sz, uint8_t *d_out, uint64_t out_cap, int32_t *h_status,
                                     uint64_t *h_out_len)
{
    if (!c || !h_out_len) return QZD_ERR_PARAM;
    *h_out_len = 0;
    if (nblocks == 0) return QZD_OK;
    if (!d_comp || !d_out || !h_records || block_sz == 0 || block_sz > 512u * 1024u) return QZD_ERR_PARAM;
    hipSetDevice(c->device);
    std::vector<int32_t> status(nblocks, 0);
    bool bad = false;
    for (uint32_t k = 0; k < nblocks; k++) {
        const qzd_blockrec &r = h_records[k];
        if (r.offset > comp_len || r.size > comp_len - r.offset || (!r.flags && r.size > block_sz)) { status[k] = -3; bad = true; }
        else if (!r.flags && k + 1 < nblocks && r.size != block_sz) { status[k] = -1; bad = true; }
    }
    if (bad) { if (h_status) memcpy(h_status, status.data(), (size_t)nblocks * 4); return QZD_ERR_DATA; }
    /* every block but the last is block_sz bytes, the last at least one (compressed: as many as there is room for, up to a block) */
    const uint64_t before = (uint64_t)(nblocks - 1) * block_sz;
    const qzd_blockrec &lr = h_records[nblocks - 1];
    if (out_cap < before + (lr.flags ? 0u : lr.size)) { snprintf(c->err, sizeof(c->err), "destination too small"); return QZD_ERR_DSTCAP; }
    const uint32_t last_cap = (uint32_t)(out_cap - before < block_sz ? out_cap - before : block_sz);

    std::vector<qzd_infseg> segs; std::vector<uint32_t> seg_blk;
    std::vector<qzk_copyjob> jobs;
    for (uint32_t k = 0; k < nblocks; k++) {
        const qzd_blockrec &r = h_records[k];
        if (r.flags) {
            qzd_infseg g; g.in_off = r.offset; g.out_off = (uint64_t)k * block_sz; g.in_len = r.size;
            g.out_cap = k + 1 < nblocks ? block_sz : last_cap; g.flags = 0; g.pad = r.size;
            segs.push_back(g); seg_blk.push_back(k);
        } else if (r.size) {
            qzk_copyjob j; j.in_off = r.offset; j.out_off = (uint64_t)k * block_sz; j.len = r.size; j.pad = 0;
            jobs.push_back(j);
        }
    }
    std::vector<uint32_t> out_len(nblocks);
    for (uint32_t k = 0; k < nblocks; k++) out_len[k] = h_records[k].flags ? 0 : h_records[k].size;
    bool cap_err = false;
    if (!segs.empty()) {
        std::vector<qzd_infres> res(segs.size());
        int rc = qzd_inflate_segments(c, d_comp, d_out, segs.data(), (uint32_t)segs.size(), res.data());
        if (rc) return rc;
        for (size_t i = 0; i < segs.size(); i++) {
            const uint32_t k = seg_blk[i];
            out_len[k] = res[i].out_len;
            if (res[i].status == -2 && k + 1 == nblocks && last_cap < block_sz) { status[k] = -2; cap_err = true; }
            else if (res[i].status != 0 || res[i].in_used != segs[i].in_len || (k + 1 < nblocks && res[i].out_len != block_sz)) { status[k] = -1; bad = true; }
        }
    }
    /* scratch of this call's own kernels: copy jobs, ranges, hashes (qzd_inflate_segments is done with its own by now) */
    const size_t jb = jobs.size() * sizeof(qzk_copyjob), rb = (size_t)nblocks * sizeof(qzk_mrange), hb = (size_t)nblocks * 4;
    int rc = meta_reserve(c, carved(jb) + carved(rb) + carved(hb));
    if (rc) return rc;
    uint8_t *p = c->d_meta;
    qzk_copyjob *d_jobs = (qzk_copyjob *)carve(&p, jb);
    qzk_mrange *d_r = (qzk_mrange *)carve(&p, rb);
    uint32_t *d_h = (uint32_t *)carve(&p, hb);
    hipStream_t st = c->st[0];
    if (!jobs.empty()) {
        HIPCHK(c, hipMemcpyAsync(d_jobs, jobs.data(), jb, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(qzk_blocks_unpack_kernel, dim3((uint32_t)jobs.size()), dim3(256), 0, st, d_comp, d_out,
                           (const qzk_copyjob *)d_jobs, (uint32_t)jobs.size());
    }
    std::vector<qzk_mrange> rng(nblocks);
    for (uint32_t k = 0; k < nblocks; k++) { rng[k].off = (uint64_t)k * block_sz; rng[k].len = status[k] ? 0 : out_len[k]; rng[k].pad = 0; }
    std::vector<uint32_t> hash(nblocks);
    HIPCHK(c, hipMemcpyAsync(d_r, rng.data(), rb, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(qzk_xxh32_ranges_kernel, dim3(nblocks), dim3(64), 0, st, (const uint8_t *)d_out, (const qzk_mrange *)d_r, nblocks, d_h);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hash.data(), d_h, hb, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (uint32_t k = 0; k < nblocks; k++)
        if (!status[k] && hash[k] != h_records[k].hash) { status[k] = -1; bad = true; }
    if (h_status) memcpy(h_status, status.data(), (size_t)nblocks * 4);
    if (cap_err) { snprintf(c->err, sizeof(c->err), "destination too small"); return QZD_ERR_DSTCAP; }
    if (bad) { snprintf(c->err, sizeof(c->err), "a block does not decode to what its record says"); return QZD_ERR_DATA; }
    *h_out_len = before + out_len[nblocks - 1];
    return QZD_OK;
}
