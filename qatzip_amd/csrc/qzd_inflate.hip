/*
 * qzd_inflate.hip — host side of the decompress half of the device C ABI.
 *
 * The software path's inflate loop (qzSWDecompressMulti / qzDeflateSWDecompress,
 * src/qatzip_sw.c:258-441,659-695) walks ONE z_stream per member serially.  On the
 * MI355X the same member is cut into independent segments at the byte-aligned
 * Z_FULL_FLUSH markers the compress side leaves after every hw_buff_sz chunk
 * (src/qatzip_sw.c:182-186), every segment is inflated by its own wave (K3), and
 * the host validates that the segments form one contiguous chain that ends in
 * BFINAL.  Marker candidates that are not real boundaries (00 00 FF FF can occur
 * inside compressed data) are discarded by that chain walk.
 *
 * Strategy per stream (qzd_inflate_stream):
 *   1. marker scan (GPU) -> sorted candidate starts; every candidate knows where the next one begins, i.e. how long
 *      it is at most compressed
 *   2a. phase A (Huffman decoding into token streams, K lanes per candidate: qzk_inflate_spec.h) over EVERY candidate,
 *      the chain walk on the host (a candidate that is no boundary drops out, every real segment gets its output
 *      offset), phase B (qzk_lz_resolve_kernel) for the real ones, range by range with the output leaving for the host
 *      behind it when the caller wants it there
 *   2b. (QATZIP_AMD_INFLATE=wave) optimistic single pass, a wave per candidate: candidate k is assumed real and to
 *      produce exactly seg_hint bytes (the session's hw_buff_sz) at k*seg_hint; validated afterwards
 *   3. otherwise two passes: count-only decode of all candidates -> chain walk + prefix sums on the host -> decode of
 *      the true segments at exact offsets
 *   4. streams whose segments reference earlier history (Z_SYNC_FLUSH producers) or have no markers are decoded by
 *      one wave straight through.
 * A member that is still in host memory (qzd_inflate_stream_from_host) goes through 1 and 2a piece by piece while it
 * arrives; whatever the pieces cannot take falls back to the list above.
 */
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <string.h>
#include <string>
#include <vector>

#include "qzd_internal.h"
#include <stdlib.h>
#include "qzk_inflate.h"
#include "qzk_inflate_lane.h"
#include "qzk_inflate_spec.h"
#include "qzk_checksum.h"
#include "qzd_inflate_plan.h"
#include <stddef.h>

/* qzd_inflate_plan.h reads the kernels' records through mirrors of its own */
static_assert(sizeof(qzp_seg) == sizeof(qzk_infseg) && offsetof(qzp_seg, in_off) == offsetof(qzk_infseg, in_off) &&
              offsetof(qzp_seg, out_off) == offsetof(qzk_infseg, out_off) && offsetof(qzp_seg, in_len) == offsetof(qzk_infseg, in_len) &&
              offsetof(qzp_seg, out_cap) == offsetof(qzk_infseg, out_cap) && offsetof(qzp_seg, flags) == offsetof(qzk_infseg, flags) &&
              offsetof(qzp_seg, pad) == offsetof(qzk_infseg, pad), "qzp_seg mirrors qzk_infseg");
static_assert(sizeof(qzp_res) == sizeof(qzk_infres) && offsetof(qzp_res, status) == offsetof(qzk_infres, status) &&
              offsetof(qzp_res, in_used) == offsetof(qzk_infres, in_used) && offsetof(qzp_res, out_len) == offsetof(qzk_infres, out_len) &&
              offsetof(qzp_res, nblocks) == offsetof(qzk_infres, nblocks), "qzp_res mirrors qzk_infres");
static_assert(QZP_FINAL == QZK_INF_FINAL && QZP_FLUSH == QZK_INF_FLUSH && QZP_TOKSEG_BYTES == sizeof(qzk_tokseg), "qzd_inflate_plan.h's constants");

/* Which kernel for how many segments (round 4, profiles/r4_inflate_crossover.txt; segments of the bench data).
 * With a compressed-length hint per segment the two phases with K lanes per segment (qzk_inflate_spec.h) win at every size
 * measured, from one megabyte (16 segments of 64 KB: 4.7 against 9.3 ms) to four gigabytes: a segment's serial chain is cut
 * in K, and one wave per segment (K3) takes ~9-12 ms for a 64 KB segment however few there are.  Without hints (a foreign
 * stream's flush points, count-only passes) phase A is one lane per segment, and that wins from ~1000 segments on (K3: 17 ms
 * at 4096 segments of 64 KB, 27 at 8192 - the CUs' scalar units; 128 KB segments: 24 ms either way at 2048, 30 against 55 at 8192). */
#define QZD_LANE_MIN_SEGS 1024u
#define QZD_LANE_MIN_SEGS_BIG 2048u
#define QZD_LANE_MIN(seg_bytes) ((seg_bytes) <= 65536u + 64u ? QZD_LANE_MIN_SEGS : QZD_LANE_MIN_SEGS_BIG)
#define QZD_LANE_SEGS_PER_WAVE 16u
/* lanes per segment of phase A (QATZIP_AMD_INFLATE_K = 1, 4, 8, 16, 32 overrides; 1 = the serial phase A).  The lanes
 * of a segment share its tables in LDS, start at evenly spaced bits and fall into step with each other: more lanes, shorter
 * chains and more waves, but more bits decoded twice.  Round 6 measured the table again with three waves a SIMD to choose from
 * (profiles/r6_phaseA_order.txt, phase A in ms at 2 / 3 waves a SIMD):
 *     segments of 64 KB      four lanes     eight          sixteen        thirty-two
 *      1024 ( 64 MiB)         8.9            5.7            3.8 / 3.7      - / 3.4
 *      8192 (512 MiB)        12.2            7.8            6.0 / 5.8      - / 6.5
 *     16384 (  1 GiB)        12.0            8.0            6.2 / 6.4      - / 8.9
 *     32768 (  2 GiB)        13.0           10.3 / 10.3    10.0 / 8.7      - / 12.8
 *     65536 (  4 GiB)        17.6           18.7 / 15.6    21.1 / 17.3     - / 22.3
 *   1 GiB of 128 KB: sixteen 10.5; of 512 KB: thirty-two 18.9 (sixteen 35); of 16 KB (65536 segments): four 5.8, eight 7.4.
 * So: segments above 16 KB take sixteen lanes up to 32768 of them (thirty-two when they are above 128 KB and few) and eight
 * beyond; segments of 16 KB and less - sixteen lanes would get under a hundred bytes each - eight up to 16384, four beyond.
 * (Round 4 kept sixteen lanes from segments above 256 KB: twenty blocks of sixteen pieces outgrew a piece list of 160 and came
 * back through the serial kernel; the list holds 640 now.) */
#define QZD_SPEC_LANES 4u
#define QZD_SPEC_LANES_FEW 8u
#define QZD_SPEC_FEW_SEGS 16384u
#define QZD_SPEC_FEW_SEGS_BIG 32768u
#define QZD_SPEC_LANES_FEWER 16u
#define QZD_SPEC_FEWER_SEGS 8192u
static uint32_t spec_lanes(const qzk_infseg *hs, uint32_t nsegs)
{
    const bool big = hs[0].out_cap > 16384u + 64u, upto512 = hs[0].out_cap <= 524288u + 64u;
    uint32_t K = nsegs <= QZD_SPEC_FEWER_SEGS && hs[0].out_cap > 131072u + 64u && upto512 ? 32u
               : big && upto512 && nsegs <= QZD_SPEC_FEW_SEGS_BIG ? QZD_SPEC_LANES_FEWER
               : big ? QZD_SPEC_LANES_FEW
               : nsegs <= QZD_SPEC_FEW_SEGS ? QZD_SPEC_LANES_FEW : QZD_SPEC_LANES;
    const char *ke = getenv("QATZIP_AMD_INFLATE_K");
    if (ke) { int v = atoi(ke); if (v == 1 || v == 4 || v == 8 || v == 16 || v == 32) K = (uint32_t)v; }
    /* it needs a compressed-length hint (qzk_infseg.pad) and segments that write output and begin with no history */
    for (uint32_t i = 0; i < nsegs && K > 1; i++)
        if ((hs[i].flags & (QZK_INF_COUNT_ONLY | QZK_INF_THROUGH_FLUSH)) || hs[i].pad == 0) K = 1;
    return K;
}
/* two phases or a wave per segment? (QATZIP_AMD_INFLATE = lane / wave overrides) */
static bool use_lanes(uint32_t K, uint32_t nsegs, uint32_t seg_bytes)
{
    const char *force = getenv("QATZIP_AMD_INFLATE");
    if (force) return force[0] == 'l';
    return K > 1 || nsegs >= QZD_LANE_MIN(seg_bytes);
}
#define QZD_SO_PARTS 8u             /* output ranges a streamed decode is resolved and sent in */

/* positions p (relative to d_src) such that src[p-4..p) == 00 00 FF FF.  A thread takes sixteen byte positions a trip:
 * five dwords (the last one for the three bytes that reach into the next piece), sixteen funnel shifts - a quarter of
 * the load instructions of one dword per position (0.74 -> ~0.3 ms for the 0.8 GB of a 2 GiB call). */
#ifdef QZK_SPEC_PROF
extern __device__ unsigned long long qzk_stamp[8];
#endif
__global__ void qzk_marker_kernel(const uint8_t *src, uint64_t n, uint32_t *list, uint32_t cap, uint32_t *count)
{
#ifdef QZK_SPEC_PROF
    if ((threadIdx.x & 63) == 0) { atomicMin(&qzk_stamp[0], (unsigned long long)__builtin_amdgcn_s_memrealtime()); }
#endif
    /* a lane takes the sixteen positions [b, b + 16): their dwords are the sixteen bytes it loads (two 8-byte loads, any
     * alignment) and the first dword of the NEXT lane's sixteen, which comes through a cross-lane read - the wave's last lane
     * loads it.  Bytes behind n read as 0.  (Round 5; five dword loads a lane before.  The kernel's time did not move -
     * 0.79 ms for the 1.6 GB of a 4 GiB call, 2 TB/s, either way: a wave has one trip's loads in flight and waits for them,
     * it is the latency of a trip that bounds it, not the number of load instructions.  More trips in flight is what is left.) */
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 16;
    for (uint64_t b0 = ((uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u)) * 16; b0 + 4 <= n; b0 += stride) {      /* (the same trips for a wave's lanes) */
        const uint64_t b = b0 + (uint64_t)lane * 16;
        uint32_t d[5];
        if (b + 16 <= n) {
            const uint64_t lo = qzk_ld64u(src + b), hi = qzk_ld64u(src + b + 8);
            d[0] = (uint32_t)lo; d[1] = (uint32_t)(lo >> 32); d[2] = (uint32_t)hi; d[3] = (uint32_t)(hi >> 32);
        } else {
            for (int k = 0; k < 4; k++) {
                d[k] = 0;
                for (int j = 0; j < 4; j++) if (b + 4 * k + j < n) d[k] |= (uint32_t)src[b + 4 * k + j] << (8 * j);
            }
        }
        d[4] = qz_shfl(d[0], (int)((lane + 1u) & 63u));
        if (lane == 63u) {
            d[4] = 0;
            if (b + 20 <= n) d[4] = qz_ld32(src + b + 16);
            else for (int j = 0; j < 4; j++) if (b + 16 + j < n) d[4] |= (uint32_t)src[b + 16 + j] << (8 * j);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t w = (k & 3) ? __builtin_amdgcn_alignbyte(d[k / 4 + 1], d[k / 4], (uint32_t)(k & 3)) : d[k / 4];
            if (w == 0xFFFF0000u && b + k + 4 <= n) {
                uint32_t i = atomicAdd(count, 1u);
                if (i < cap) list[i] = (uint32_t)(b + k + 4);
            }
        }
    }
}
/* the scan as it was through round 4 (five dword loads a lane): QATZIP_AMD_MARKER_CHECK=1 runs it beside the one above and
 * compares what they find (tests/test_gpu_inflate.py) */
__global__ void qzk_marker_ref_kernel(const uint8_t *src, uint64_t n, uint32_t *list, uint32_t cap, uint32_t *count)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 16;
    for (uint64_t b = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; b + 4 <= n; b += stride) {
        uint32_t d[5];
        for (int k = 0; k < 5; k++) {
            d[k] = 0;
            if (b + 4 * k + 4 <= n) d[k] = qz_ld32(src + b + 4 * k);
            else for (int j = 0; j < 4; j++) if (b + 4 * k + j < n) d[k] |= (uint32_t)src[b + 4 * k + j] << (8 * j);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t w = (k & 3) ? __builtin_amdgcn_alignbyte(d[k / 4 + 1], d[k / 4], (uint32_t)(k & 3)) : d[k / 4];
            if (w == 0xFFFF0000u && b + k + 4 <= n) {
                uint32_t i = atomicAdd(count, 1u);
                if (i < cap) list[i] = (uint32_t)(b + k + 4);
            }
        }
    }
}

/* Control data between the host's pinned staging and the device (segment records in, results and candidate lists out):
 * moved by a small KERNEL, not by the copy engines.  A copy engine takes its copies in order, so a 16-byte result queued
 * behind a quarter of a gigabyte of output on its way to the host arrived when that had arrived - the piece-wise decode
 * (qzd_inflate_stream_from_host) stood still behind its own output for 30 ms.  Both ends are multiples of four bytes;
 * the host side is hipHostMalloc memory, which the device reads and writes in place. */
__global__ void qzk_ctl_copy_kernel(uint32_t *dst, const uint32_t *src, size_t n4)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
/* The sub-stream descriptors of a call whose segments are all of one size (every call of fixed hw_buff_sz chunks): segment i's
 * lane j has the region [i * seg + pre[j], + len[j]) - written here instead of being built on the host and sent across (sixteen
 * bytes a lane: 8 MB for the bench's 4 GiB call, a third of a millisecond of PCIe and as much of host loop before phase A). */
struct qzk_tsfill { uint64_t pre[32], len[32]; uint64_t seg; };
__global__ void qzk_ts_fill_kernel(qzk_tokseg *ts, uint32_t nsegs, uint32_t K, const qzk_tsfill F)
{
    const size_t n = (size_t)nsegs * K;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
        const uint64_t i = t / K, j = t % K, a = i * F.seg + F.pre[j];
        ts[t].lit_off = a; ts[t].seq_off = (a + F.len[j]) / 8;
    }
}
static hipError_t ctl_copy(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    if (!bytes) return hipSuccess;
    const size_t n4 = (bytes + 3) / 4;
    const unsigned blocks = (unsigned)std::min<size_t>((n4 + 255) / 256, 256);
    hipLaunchKernelGGL(qzk_ctl_copy_kernel, dim3(blocks), dim3(256), 0, st, (uint32_t *)dst, (const uint32_t *)src, n4);
    return hipGetLastError();
}

/* ---- two_phase(): phase A over nsegs segments, in steps ---- */
/* the pinned mirror of a call (tp_mirror, qzd_inflate_plan.h) as pointers: everything that crosses PCIe here goes through
 * it (a copy from or to pageable memory is staged by the runtime in pieces, each with its own wait: a quarter of a
 * millisecond per megabyte, four times per call, between two kernels) */
struct tp_host { qzk_infseg *segs; qzk_infres *res; qzk_tokseg *ts; uint32_t *ord; };
static tp_host tp_host_of(qzd_ctx *c, const tp_mirror &M)
{
    return tp_host{(qzk_infseg *)c->h_aux, (qzk_infres *)(c->h_aux + M.o_res), (qzk_tokseg *)(c->h_aux + M.o_ts), (uint32_t *)(c->h_aux + M.o_ord)};
}
/* the device arrays of a call: records and results in the aux scratch, the rest carved from the big one */
struct tp_dev {
    qzk_infseg *segs; qzk_infres *res; qzk_inf_tab *tab; qzk_tokseg *ts; qzk_chain *ch; qzk_rec *rec;
    uint8_t *lit; qzk_seq *seq; uint32_t *ord;
};

/* Region plan.  Every sub-stream is one region of the scratch, literals up from its first byte, sequences down from its end
 * (qzk_inflate_lane.h).  K == 1: a region that holds any segment; K > 1: regions sized by need (qzk_inflate_spec.h), and
 * behind them R whole-segment regions for the segments that kernel hands back to the serial one.
 * uniform - one size for all (no count-only segments, K <= 32): the descriptors are written on the device from F
 * (qzk_ts_fill_kernel), and the host's copy of them only if a segment is handed back (fill_host). */
struct tp_plan {
    bool uniform; qzk_tsfill F;
    uint64_t arena;                 /* bytes of all regions, the hand-back area included */
    uint64_t hb0, hb_rg; uint32_t R;        /* the hand-back area: R regions of hb_rg bytes from hb0 on */
};
/* leaves the plan in *pl and, when it is not uniform, every sub-stream's descriptor in tsv */
static int plan_regions(qzd_ctx *c, const qzk_infseg *hs, uint32_t nsegs, uint32_t K, qzk_tokseg *tsv, tp_plan *pl)
{
    uint64_t arena = 0, max_cap = 0;
    qzk_tsfill &F = pl->F;
    bool uniform = nsegs > 0 && K <= 32;
    for (uint32_t i = 0; i < nsegs && uniform; i++) uniform = !(hs[i].flags & QZK_INF_COUNT_ONLY) && hs[i].out_cap == hs[0].out_cap;
    if (uniform) {
        F.seg = 0; max_cap = hs[0].out_cap;
        for (uint32_t j = 0; j < K; j++) {
            F.len[j] = K == 1 ? QZK_TOK_REGION(hs[0].out_cap) : QZK_SPEC_REGION(hs[0].out_cap, K, j);
            F.pre[j] = F.seg; F.seg += F.len[j];
        }
        arena = (uint64_t)nsegs * F.seg;
    } else
    for (uint32_t i = 0; i < nsegs; i++) {
        const bool writes = !(hs[i].flags & QZK_INF_COUNT_ONLY);
        if (writes && hs[i].out_cap > max_cap) max_cap = hs[i].out_cap;
        for (uint32_t j = 0; j < K; j++) {
            const uint64_t rg = !writes ? 0 : K == 1 ? QZK_TOK_REGION(hs[i].out_cap) : QZK_SPEC_REGION(hs[i].out_cap, K, j);
            tsv[(size_t)i * K + j].lit_off = arena; tsv[(size_t)i * K + j].seq_off = (arena + rg) / 8;
            arena += rg;
        }
    }
    pl->uniform = uniform;
    pl->R = K == 1 ? 0u : std::min<uint32_t>(nsegs, QZK_SPEC_HANDBACK(nsegs));
    pl->hb0 = arena; pl->hb_rg = QZK_TOK_REGION(max_cap);
    pl->arena = arena + (uint64_t)pl->R * pl->hb_rg;
    /* sequences grow down from a region's end in 16-byte stores (qzk_inflate_lane.h): every region starts and ends 16-aligned */
    bool aligned = ((pl->hb0 | pl->hb_rg) & 15) == 0;
    if (uniform) for (uint32_t j = 0; j < K; j++) aligned &= ((F.pre[j] | F.len[j] | F.seg) & 15) == 0;
    else for (size_t i = 0; i < (size_t)nsegs * K; i++) aligned &= ((tsv[i].lit_off & 15) | (tsv[i].seq_off & 1)) == 0;
    if (!aligned) { snprintf(c->err, sizeof(c->err), "inflate: a token region is not 16-byte aligned"); return QZD_ERR_PARAM; }
    return QZD_OK;
}
/* a uniform plan's layout in the host's table */
static void fill_host(const tp_plan &pl, qzk_tokseg *tsv, uint32_t nsegs, uint32_t K)
{
    for (uint32_t i = 0; i < nsegs; i++)
        for (uint32_t j = 0; j < K; j++) {
            const uint64_t a = (uint64_t)i * pl.F.seg + pl.F.pre[j];
            tsv[(size_t)i * K + j].lit_off = a; tsv[(size_t)i * K + j].seq_off = (a + pl.F.len[j]) / 8;
        }
}

/* Leaves c->d_big with `need` bytes or more, or answers QZD_ERR_NOMEM (c->err untouched: the caller may have another way).
 * The scratch grows with the largest call and shrinks again when EIGHT calls in a row have needed less than a quarter of it
 * (a 4 GiB decode leaves gigabytes behind; a session of small calls gives them back, one that alternates large and small
 * ones keeps them - every change is a free and an allocation).  What runs on the scratch runs on this context's
 * streams: they are waited for, not the device - helper contexts decode other pieces meanwhile */
static int big_reserve(qzd_ctx *c, size_t need, hipStream_t st)
{
    if (c->big_cap > ((size_t)1 << 30) && need * 4 < c->big_cap) c->big_small++; else c->big_small = 0;
    if (need <= c->big_cap && c->big_small < 8) return QZD_OK;
    c->big_small = 0;
    hipStreamSynchronize(st); hipStreamSynchronize(c->st_out);
    if (c->d_big) hipFree(c->d_big);
    c->d_big = NULL; c->big_cap = 0;
    /* QATZIP_AMD_SCRATCH_MAX=<bytes>: a ceiling for this scratch (tests: the paths a failed allocation takes) */
    const char *cap_e = getenv("QATZIP_AMD_SCRATCH_MAX");
    const bool refused = cap_e && need > (size_t)strtoull(cap_e, NULL, 10);
    if (refused || hipMalloc(&c->d_big, need) != hipSuccess) {
        (void)hipGetLastError();
        c->d_big = NULL;
        return QZD_ERR_NOMEM;
    }
    c->big_cap = need;
    return QZD_OK;
}

#ifndef QZD_TOK_OCC
#define QZD_TOK_OCC 2           /* waves per SIMD of phase A's sixteen-lane workgroups: what their root tables leave room for in LDS */
#endif
/* launches the serial phase A over all segments (order NULL) or over `count` of them picked by index; it fills sub-stream 0 */
static void tok_launch(hipStream_t st, const uint8_t *d_comp, const tp_dev &D, uint32_t nsegs, uint32_t K, const uint32_t *order, uint32_t count)
{
    /* segments per single-wave workgroup of the serial phase A: each lane keeps 1.25 KiB of root tables in LDS, and partly
     * filled waves give the serial decode loops more waves to hide behind (measured in DESIGN.md K3b) */
    uint32_t lpw = QZD_LANE_SEGS_PER_WAVE;
    const char *le = getenv("QATZIP_AMD_INFLATE_LPW");
    if (le) { int v = atoi(le); if (v == 8 || v == 16 || v == 32 || v == 64) lpw = (uint32_t)v; }
    const char *oe = getenv("QATZIP_AMD_INFLATE_OCC");
    const int occ = oe ? atoi(oe) : 0;
    const dim3 grid(((order ? count : nsegs) + lpw - 1) / lpw), blk(lpw);
#define QZD_TOK_LAUNCH(N, W) hipLaunchKernelGGL((qzk_inflate_tok_kernel<N, W>), grid, blk, 0, st, d_comp, D.segs, D.res, nsegs, D.tab, \
                                               D.ts, D.lit, D.seq, D.ch, order, count, K)
    switch (lpw) {
    case 8: if (occ == 2) QZD_TOK_LAUNCH(8, 2); else QZD_TOK_LAUNCH(8, 4); break;
    case 32: QZD_TOK_LAUNCH(32, 1); break;
    case 64: QZD_TOK_LAUNCH(64, 1); break;
    default: QZD_TOK_LAUNCH(16, QZD_TOK_OCC);
    }
#undef QZD_TOK_LAUNCH
}
/* launches the speculative phase A: K lanes per segment, 64 / K segments per wave */
static void spec_launch(qzd_ctx *c, hipStream_t st, const uint8_t *d_comp, const tp_dev &D, const qzk_infseg *hs, uint32_t nsegs, uint32_t K)
{
    const uint32_t spw = 64 / K;
    const dim3 grid((nsegs + spw - 1) / spw), blk(64);
    static std::atomic<uint64_t> spec_epoch{0};                     /* tags the marks of a launch: scratch left by an earlier one is not mistaken for them */
    const uint64_t epoch = ++spec_epoch;
    /* how far a block's last lane may run beyond its share before the rest is shared out again (a round more): segments
     * above 64 KB hold several blocks of very different length and pay for every lane left alone; small launches end
     * with their longest lane; a full launch of 64 KB segments is better off without the extra rounds
     * (profiles/r4_inflate_crossover.txt) */
    uint32_t over = hs[0].out_cap > 65536u + 64u ? 2u : nsegs <= 4096u ? 1u : 1000u;
    const char *ov = getenv("QATZIP_AMD_INFLATE_OVER");
    if (ov && atoi(ov) > 0) over = (uint32_t)atoi(ov);
    /* waves per SIMD (qzk_inflate_spec.h): three - with a third of the registers spilled - pay from the third round of
     * resident waves on (QATZIP_AMD_INFLATE_OCC=2 / 3 overrides) */
    const char *oe = getenv("QATZIP_AMD_INFLATE_OCC");
    const int occ = oe ? atoi(oe) : 0;
    int socc = grid.x > 16u * c->cus && K != 4 ? 3 : 2;
    if (occ == 2 || (occ == 3 && K != 4)) socc = occ;
#define QZD_SPEC_LAUNCH(N, W) hipLaunchKernelGGL((qzk_inflate_spec_kernel<N, W>), grid, blk, 0, st, d_comp, D.segs, D.res, nsegs, D.tab, \
                                             D.ts, D.lit, D.seq, D.ch, D.rec, epoch, over)
    switch (K) {
    case 4: QZD_SPEC_LAUNCH(4, 2); break;
    case 16: if (socc == 3) QZD_SPEC_LAUNCH(16, 3); else QZD_SPEC_LAUNCH(16, 2); break;
    case 32: if (socc == 3) QZD_SPEC_LAUNCH(32, 3); else QZD_SPEC_LAUNCH(32, 2); break;
    default: if (socc == 3) QZD_SPEC_LAUNCH(8, 3); else QZD_SPEC_LAUNCH(8, 2);
    }
#undef QZD_SPEC_LAUNCH
}

/* What the K-lane kernel hands back (QZK_INF_ESPEC: a sub-stream outgrew its scratch, too many pieces) goes through the
 * serial phase A, into one of the R whole-segment regions of the hand-back area behind the sub-streams (the K-lane
 * regions are sized by need: lane 0's holds half a segment or less from K = 8 on).  Leaves the results of the K-lane
 * launch in H.res and their number of hand-backs in *nredo; up to R of them are launched again, more are the caller's. */
static int handback_redo(qzd_ctx *c, hipStream_t st, const uint8_t *d_comp, const tp_plan &pl, const tp_host &H, const tp_dev &D,
                         uint32_t nsegs, uint32_t K, uint32_t *nredo_out)
{
    HIPCHK(c, ctl_copy(H.res, D.res, (size_t)nsegs * sizeof(qzk_infres), st));
    HIPCHK(c, hipStreamSynchronize(st));
    uint32_t nredo = 0;
    for (uint32_t i = 0; i < nsegs; i++) if (H.res[i].status == QZK_INF_ESPEC) H.ord[nredo++] = i;
    if (nredo && getenv("QATZIP_AMD_TRACE")) {
        uint32_t hist[64] = {0};
        for (uint32_t i = 0; i < nredo; i++) { const uint32_t w = H.res[H.ord[i]].nblocks; hist[w < 64 ? w : 63]++; }
        fprintf(stderr, "[two_phase] K=%u: %u of %u segments handed back to the serial kernel; reasons:", K, nredo, nsegs);
        for (int k = 0; k < 64; k++) if (hist[k]) fprintf(stderr, " %d:%u", k, hist[k]);
        fprintf(stderr, "\n");
    }
    c->inf_handback_acc += nredo;
    *nredo_out = nredo;
    if (nredo == 0 || nredo > pl.R) return QZD_OK;
    if (pl.uniform) fill_host(pl, H.ts, nsegs, K);
    for (uint32_t k = 0; k < nredo; k++) {
        qzk_tokseg &t0 = H.ts[(size_t)H.ord[k] * K];
        t0.lit_off = pl.hb0 + (uint64_t)k * pl.hb_rg; t0.seq_off = (pl.hb0 + (uint64_t)(k + 1) * pl.hb_rg) / 8;
    }
    HIPCHK(c, ctl_copy(D.ts, H.ts, (size_t)nsegs * K * sizeof(qzk_tokseg), st));
    HIPCHK(c, ctl_copy(D.ord, H.ord, (size_t)nredo * 4, st));
    tok_launch(st, d_comp, D, nsegs, K, D.ord, nredo);
    return QZD_OK;
}

/* Phase B of the last phase A (c->tp) over `parts` ranges of the output: order[0 .. count) are the segments to resolve in
 * output order (the same list stands at c->tp.ord on the device), range p is a launch of its own.  With h_dst every range
 * leaves for the host on out_st behind its launch's event while the next one is being resolved; while_leaving is called once
 * the copies are queued, before they are waited for; c->so_sent = the end of what went out.  Leaves c->ev[1][2] behind the
 * last launch.  (Whether the ranges are what the caller wanted is decided afterwards, from the results; a decode that turns
 * out wrong is simply copied again as a whole.) */
static int resolve_ranges(qzd_ctx *c, hipStream_t st, hipStream_t out_st, const uint8_t *d_comp, uint8_t *d_out, const qzk_infseg *hs,
                          const uint32_t *order, uint32_t count, uint32_t parts, uint8_t *h_dst, const std::function<void()> *while_leaving)
{
    uint64_t off[QZD_SO_PARTS + 1];
    for (uint32_t p = 0; p < parts; p++) {
        const uint32_t first = (uint32_t)((uint64_t)count * p / parts), end = (uint32_t)((uint64_t)count * (p + 1) / parts);
        off[p] = hs[order[first]].out_off;
        off[p + 1] = hs[order[end - 1]].out_off + hs[order[end - 1]].out_cap;
        hipLaunchKernelGGL(qzk_lz_resolve_kernel, dim3((end - first + QZK_RES_WAVES - 1) / QZK_RES_WAVES), dim3(64 * QZK_RES_WAVES), 0, st,
                           d_comp, d_out, (const qzk_infseg *)c->tp.segs, (qzk_infres *)c->tp.res, c->tp.nsegs, (const qzk_tokseg *)c->tp.ts, c->tp.K,
                           (const uint8_t *)c->tp.lits, (const qzk_seq *)c->tp.seqs, (const qzk_chain *)c->tp.chains,
                           (const uint32_t *)(c->tp.ord + first), end - first);
        if (h_dst) HIPCHK(c, hipEventRecord(c->so_ev[p], st));
    }
    HIPCHK(c, hipEventRecord(c->ev[1][2], st));
    if (h_dst) {
        for (uint32_t p = 0; p < parts; p++) {       /* a pageable destination makes these block the host: all launches are out already */
            HIPCHK(c, hipStreamWaitEvent(out_st, c->so_ev[p], 0));
            HIPCHK(c, hipMemcpyAsync(h_dst + off[p], d_out + off[p], off[p + 1] - off[p], hipMemcpyDeviceToHost, out_st));
        }
        if (while_leaving) (*while_leaving)();
        HIPCHK(c, hipStreamSynchronize(out_st));
        c->so_sent = off[parts];
    }
    return QZD_OK;
}

/* the results of what has run on st, through the mirror into h_res */
static int fetch_results(qzd_ctx *c, qzk_infres *st_res, const qzk_infres *d_res, uint32_t nsegs, qzk_infres *h_res, hipStream_t st)
{
    const size_t rb = (size_t)nsegs * sizeof(qzk_infres);
    HIPCHK(c, ctl_copy(st_res, d_res, rb, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    memcpy(h_res, st_res, rb);
    return QZD_OK;
}

/* Two-phase inflate of nsegs segments (qzk_inflate_lane.h / qzk_inflate_spec.h).  K == 1: one lane decodes a whole
 * segment; K > 1: K lanes per segment decode speculatively, and whatever that kernel hands back (QZK_INF_ESPEC: stored
 * or several blocks, bad data, ...) goes through the K == 1 launch afterwards.  h_res receives every result. */
static int two_phase(qzd_ctx *c, const uint8_t *d_comp, uint8_t *d_out, const qzk_infseg *hs, uint32_t nsegs,
                     qzk_infres *h_res, uint32_t K, hipStream_t st, bool run_b = true)
{
    const tp_mirror M = tp_mirror_of(nsegs, K);
    int rc = qzd_aux_reserve(c, M.bytes + 64);
    if (rc) return rc;
    const tp_host H = tp_host_of(c, M);
    const size_t sb = (size_t)nsegs * sizeof(qzk_infseg);
    memcpy(H.segs, hs, sb);
    tp_plan pl;
    rc = plan_regions(c, hs, nsegs, K, H.ts, &pl);
    if (rc) return rc;
    const size_t tabb = ((size_t)nsegs * sizeof(qzk_inf_tab) + 255) & ~(size_t)255;
    const size_t tsb = ((size_t)nsegs * K * sizeof(qzk_tokseg) + 255) & ~(size_t)255;
    const size_t chb = ((size_t)nsegs * sizeof(qzk_chain) + 255) & ~(size_t)255;
    const size_t rcb = K == 1 ? 0 : (((size_t)nsegs * K * QZK_SPEC_NREC * sizeof(qzk_rec) + 255) & ~(size_t)255);
    const size_t litb = (pl.arena + 1023) & ~(uint64_t)255;         /* (one arena; phase B reads whole 16-byte rows past a region's literals) */
    const size_t ordb = ((size_t)nsegs * 4 + 255) & ~(size_t)255;
    const size_t need = tabb + tsb + chb + rcb + litb + ordb + 256;
    /* output streaming: only the plain decode of a whole member (every segment writes, known output offsets).  It is reached
     * through path 2b alone, with a launch of QZD_LANE_MIN_SEGS segments or more: a token scratch refused a moment earlier */
    const bool stream_out = run_b && c->so_host && c->so_nat && nsegs >= QZD_LANE_MIN_SEGS;
    if (big_reserve(c, need, st) != QZD_OK) {
        /* not enough device memory for K sub-streams per segment: one per segment needs a third of it; after that the
         * callers take the wave-per-segment kernel, which needs none */
        if (K > 1) return two_phase(c, d_comp, d_out, hs, nsegs, h_res, 1, st, run_b);
        snprintf(c->err, sizeof(c->err), "inflate: %zu bytes of decode scratch are not available", need);
        return QZD_ERR_NOMEM;
    }
    tp_dev D;
    uint8_t *pb = c->d_big;
    D.segs = (qzk_infseg *)c->d_aux; D.res = (qzk_infres *)(c->d_aux + M.o_res);
    D.tab = (qzk_inf_tab *)pb; pb += tabb;
    D.ts = (qzk_tokseg *)pb; pb += tsb;
    D.ch = (qzk_chain *)pb; pb += chb;
    D.rec = (qzk_rec *)pb; pb += rcb;
    D.lit = pb; pb += litb;
    D.seq = (qzk_seq *)D.lit;                           /* the same arena: a region's sequences count down from its end */
    D.ord = (uint32_t *)pb;
    HIPCHK(c, ctl_copy(D.segs, H.segs, sb, st));
    if (pl.uniform) {
        hipLaunchKernelGGL(qzk_ts_fill_kernel, dim3((unsigned)std::min<size_t>(((size_t)nsegs * K + 255) / 256, 1024)), dim3(256), 0, st, D.ts, nsegs, K, pl.F);
        HIPCHK(c, hipGetLastError());
    } else HIPCHK(c, ctl_copy(D.ts, H.ts, (size_t)nsegs * K * sizeof(qzk_tokseg), st));
    HIPCHK(c, hipEventRecord(c->ev[1][1], st));
    bool res_fresh = false;                                         /* the host's copy of the results is current (nothing ran since it was taken) */
    if (K == 1) tok_launch(st, d_comp, D, nsegs, K, NULL, 0);
    else {
        spec_launch(c, st, d_comp, D, hs, nsegs, K);
        uint32_t nredo = 0;
        rc = handback_redo(c, st, d_comp, pl, H, D, nsegs, K, &nredo);
        if (rc) return rc;
        if (nredo > pl.R) {                                         /* more than the hand-back area holds: this data is not what K lanes are for */
            c->inf_k1rerun_acc++;
            return two_phase(c, d_comp, d_out, hs, nsegs, h_res, 1, st, run_b);
        }
        res_fresh = nredo == 0;
    }
    HIPCHK(c, hipEventRecord(c->ev[1][0], st));
    c->tp.segs = D.segs; c->tp.res = D.res; c->tp.ts = D.ts; c->tp.lits = D.lit; c->tp.seqs = D.seq; c->tp.chains = D.ch;
    c->tp.ord = D.ord; c->tp.nsegs = nsegs; c->tp.K = K;
    float t = 0;
    if (!run_b) {
        /* phase A only: its results say which candidates are real segments and where their output belongs;
         * two_phase_resolve() runs phase B once the host has decided */
        if (!res_fresh) rc = fetch_results(c, H.res, D.res, nsegs, h_res, st);
        else {
            HIPCHK(c, hipEventSynchronize(c->ev[1][0]));            /* (the stream stood still when it was recorded) */
            HIPCHK(c, hipGetLastError());
            memcpy(h_res, H.res, (size_t)nsegs * sizeof(qzk_infres));
        }
        if (rc) return rc;
        if (hipEventElapsedTime(&t, c->ev[1][1], c->ev[1][0]) == hipSuccess) c->inf_ms[3] += t;    /* phase A's kernel(s) */
        return QZD_OK;
    }
    if (stream_out) {
        HIPCHK(c, hipStreamSynchronize(st));                        /* the redo list in H.ord may still be on its way to the device */
        memcpy(H.ord, c->so_nat, (size_t)nsegs * 4); HIPCHK(c, ctl_copy(D.ord, H.ord, (size_t)nsegs * 4, st));
        /* up to QZD_SO_PARTS ranges of the output, in output order (two_phase_resolve() counts the real segments, this all of them) */
        rc = resolve_ranges(c, st, c->st_out, d_comp, d_out, hs, c->so_nat, nsegs, std::min<uint32_t>(QZD_SO_PARTS, std::max<uint32_t>(1u, nsegs / 4096u)),
                            c->so_host, NULL);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(qzk_lz_resolve_kernel, dim3((nsegs + QZK_RES_WAVES - 1) / QZK_RES_WAVES), dim3(64 * QZK_RES_WAVES), 0, st,
                           d_comp, d_out, D.segs, D.res, nsegs, D.ts, K, D.lit, D.seq, D.ch, (const uint32_t *)NULL, 0u);
        HIPCHK(c, hipEventRecord(c->ev[1][2], st));
    }
    rc = fetch_results(c, H.res, D.res, nsegs, h_res, st);
    if (rc) return rc;
    if (hipEventElapsedTime(&t, c->ev[1][0], c->ev[1][2]) == hipSuccess) c->inf_ms[2] += t;     /* phase B share */
    if (hipEventElapsedTime(&t, c->ev[1][1], c->ev[1][0]) == hipSuccess) c->inf_ms[3] += t;     /* phase A's kernel(s) */
    return QZD_OK;
}

/* Phase B for the segments of the last two_phase(run_b = false) call that the host found to be real: hs = the same
 * records with their final out_off (candidates that are no segments carry QZK_INF_COUNT_ONLY and are skipped),
 * h_order = the real ones in output order.  With h_dst the output leaves for the host range by range behind the launches.
 * Results (phase B can still find a bad distance) come back in h_res. */
static int two_phase_resolve(qzd_ctx *c, const uint8_t *d_comp, uint8_t *d_out, const qzk_infseg *hs, uint32_t nsegs,
                             const uint32_t *h_order, uint32_t count, qzk_infres *h_res, uint8_t *h_dst, hipStream_t st, hipStream_t out_st = NULL,
                             const std::function<void()> *while_leaving = NULL /* called once the output's copies are queued, before they are waited for */)
{
    if (!out_st) out_st = c->st_out;
    if (nsegs != c->tp.nsegs || count == 0) return QZD_ERR_PARAM;
    const tp_mirror M = tp_mirror_of(nsegs, c->tp.K);               /* as the phase A that ran laid it out: the same nsegs, its K */
    if (M.bytes > c->aux_cap) return QZD_ERR_PARAM;
    const tp_host H = tp_host_of(c, M);
    const size_t sb = (size_t)nsegs * sizeof(qzk_infseg);
    memcpy(H.segs, hs, sb);
    memcpy(H.ord, h_order, (size_t)count * 4);
    HIPCHK(c, ctl_copy(c->tp.segs, H.segs, sb, st));
    HIPCHK(c, ctl_copy(c->tp.ord, H.ord, (size_t)count * 4, st));
    HIPCHK(c, hipEventRecord(c->ev[1][0], st));
    /* ranges of the output that leave one behind the other: a launch lasts as long as its slowest segment (~1 ms for 64 KB),
     * so a range is worth a launch of its own from ~4096 segments on (eight launches over 3000 segments took 8.8 ms, one 1.3) */
    const uint32_t parts = !h_dst ? 1u : std::min<uint32_t>(QZD_SO_PARTS, std::max<uint32_t>(1u, count / 4096u));
    int rc = resolve_ranges(c, st, out_st, d_comp, d_out, hs, h_order, count, parts, h_dst, while_leaving);
    if (rc) return rc;
    rc = fetch_results(c, H.res, (const qzk_infres *)c->tp.res, nsegs, h_res, st);
    if (rc) return rc;
    float t = 0;
    if (hipEventElapsedTime(&t, c->ev[1][0], c->ev[1][2]) == hipSuccess) c->inf_ms[2] += t;
    return QZD_OK;
}

extern "C" int qzd_inflate_stats(qzd_ctx *c, uint64_t *handed_back_segments, uint64_t *k1_reruns, int reset)
{
    if (!c) return QZD_ERR_PARAM;
    if (handed_back_segments) *handed_back_segments = c->inf_handback_acc;
    if (k1_reruns) *k1_reruns = c->inf_k1rerun_acc;
    if (reset) { c->inf_handback_acc = 0; c->inf_k1rerun_acc = 0; }
    return QZD_OK;
}

extern "C" int qzd_inflate_segments(qzd_ctx *c, const uint8_t *d_comp, uint8_t *d_out, const void *h_segs,
                                    uint32_t nsegs, void *h_res)
{
    if (!c || !h_segs || !h_res) return QZD_ERR_PARAM;
    if (nsegs == 0) return QZD_OK;
    hipSetDevice(c->device);
    hipStream_t st = c->st[0];
    const qzk_infseg *hs = (const qzk_infseg *)h_segs;
    /* few segments: one wave each; thousands: the two-phase path (the wave-per-segment kernel is bound by the CU's
     * scalar unit, the lane kernels spread the serial work over the vector lanes) */
    const uint32_t K = spec_lanes(hs, nsegs);
    const bool lanes = use_lanes(K, nsegs, hs[0].out_cap);
    HIPCHK(c, hipEventRecord(c->ev[0][0], st));
    bool waves = !lanes;
    if (lanes) {
        int rc = two_phase(c, d_comp, d_out, hs, nsegs, (qzk_infres *)h_res, K, st);
        if (rc == QZD_ERR_NOMEM) waves = true;                      /* no room for the token streams: a wave per segment needs none */
        else if (rc) return rc;
    }
    if (waves) {
        const size_t sb = (size_t)nsegs * sizeof(qzk_infseg), rb = (size_t)nsegs * sizeof(qzk_infres);
        int rc = qzd_aux_reserve(c, sb + rb + 64);
        if (rc) return rc;
        qzk_infseg *d_segs = (qzk_infseg *)c->d_aux;
        qzk_infres *d_res = (qzk_infres *)(c->d_aux + ((sb + 15) & ~(size_t)15));
        HIPCHK(c, hipMemcpyAsync(d_segs, h_segs, sb, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(qzk_inflate_kernel, dim3((nsegs + QZK_INF_WAVES - 1) / QZK_INF_WAVES), dim3(64 * QZK_INF_WAVES),
                           0, st, d_comp, d_out, d_segs, d_res, nsegs);
        HIPCHK(c, hipMemcpyAsync(h_res, d_res, rb, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->ev[0][1], st));
    HIPCHK(c, hipStreamSynchronize(st));
    float t = 0;
    if (hipEventElapsedTime(&t, c->ev[0][0], c->ev[0][1]) == hipSuccess) c->inf_ms[0] += t;
    return QZD_OK;
}

extern "C" int qzd_crc32_ranges(qzd_ctx *c, const uint8_t *d_data, const void *h_ranges, uint32_t nranges,
                                uint32_t *h_crc)
{
    if (!c || !h_ranges || !h_crc) return QZD_ERR_PARAM;
    if (nranges == 0) return QZD_OK;
    hipSetDevice(c->device);
    const size_t rb = (size_t)nranges * sizeof(qzk_range), cb = (size_t)nranges * 4;
    int rc = qzd_aux_reserve(c, rb + cb + 64);
    if (rc) return rc;
    qzk_range *d_r = (qzk_range *)c->d_aux;
    const size_t o_c = (rb + 15) & ~(size_t)15;
    uint32_t *d_c = (uint32_t *)(c->d_aux + o_c);
    hipStream_t st = c->st[0];
    memcpy(c->h_aux, h_ranges, rb);                                 /* through the pinned mirror, both ways */
    HIPCHK(c, hipMemcpyAsync(d_r, c->h_aux, rb, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(c->ev[0][2], st));
    hipLaunchKernelGGL(qzk_crc_kernel, dim3(nranges), dim3(QZK_HT), 0, st, d_data, d_r, nranges, d_c);
    HIPCHK(c, hipEventRecord(c->ev[0][3], st));
    HIPCHK(c, hipMemcpyAsync(c->h_aux + o_c, d_c, cb, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(h_crc, c->h_aux + o_c, cb);
    float t = 0;
    if (hipEventElapsedTime(&t, c->ev[0][2], c->ev[0][3]) == hipSuccess) c->inf_ms[1] += t;
    return QZD_OK;
}

/* zlib adler32_combine() */
extern "C" uint32_t qzd_adler32_combine(uint32_t ad1, uint32_t ad2, uint64_t len2)
{
    const uint64_t M = 65521;
    const uint64_t a1 = ad1 & 0xffff, b1 = ad1 >> 16, a2 = ad2 & 0xffff, b2 = ad2 >> 16;
    const uint64_t a = (a1 + a2 + M - 1) % M;
    const uint64_t b = (b1 + b2 + (len2 % M) * ((a1 + M - 1) % M)) % M;
    return (uint32_t)(b << 16 | a);
}

/* Adler-32 of every chunk_sz chunk of d_data[0..n) (h_adler: one value per chunk; fold with qzd_adler32_combine) */
extern "C" int qzd_adler32_chunks(qzd_ctx *c, const uint8_t *d_data, uint64_t n, uint32_t chunk_sz, uint32_t *h_adler)
{
    if (!c || !h_adler || (n && !d_data) || chunk_sz == 0 || chunk_sz > 512 * 1024) return QZD_ERR_PARAM;
    const uint32_t nchunks = n ? (uint32_t)((n + chunk_sz - 1) / chunk_sz) : 1;
    hipSetDevice(c->device);
    int rc = qzd_aux_reserve(c, (size_t)nchunks * 4 + 64);
    if (rc) return rc;
    hipStream_t st = c->st[0];
    hipLaunchKernelGGL(qzk_adler_chunks_kernel, dim3(nchunks), dim3(QZK_HT), 0, st, d_data, n, chunk_sz, nchunks, (uint32_t *)c->d_aux);
    HIPCHK(c, hipMemcpyAsync(h_adler, c->d_aux, (size_t)nchunks * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return QZD_OK;
}

extern "C" int qzd_crc32(qzd_ctx *c, const uint8_t *d_data, uint64_t n, uint32_t *h_crc)
{
    /* CRC-32 of d_data[0..n): a workgroup per 256 KB, the values folded on the host with the multiplier of a full piece
     * computed once (qzd_crc32_fold).  No list of ranges goes to the device and the values come back through a small kernel,
     * not through the copy engine (round 5: the two copies and their waits were 0.5 ms of a 1.9 ms step at 4 GiB) */
    if (!c || !h_crc || (n && !d_data)) return QZD_ERR_PARAM;
    const uint32_t R = 256 * 1024;
    const uint32_t nr = (uint32_t)((n + R - 1) / R);
    *h_crc = 0;
    if (nr == 0) return QZD_OK;
    hipSetDevice(c->device);
    const size_t cb = (size_t)nr * 4;
    int rc = qzd_aux_reserve(c, cb + 64);
    if (rc) return rc;
    hipStream_t st = c->st[0];
    uint32_t *d_c = (uint32_t *)c->d_aux;
    HIPCHK(c, hipEventRecord(c->ev[0][2], st));
    hipLaunchKernelGGL(qzk_crc_chunks_kernel, dim3(nr), dim3(QZK_HT), 0, st, d_data, n, R, nr, d_c, (const uint32_t *)NULL);
    HIPCHK(c, hipEventRecord(c->ev[0][3], st));
    HIPCHK(c, ctl_copy(c->h_aux, d_c, cb, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    *h_crc = qzd_crc32_fold((const uint32_t *)c->h_aux, nr, R, n);
    float t = 0;
    if (hipEventElapsedTime(&t, c->ev[0][2], c->ev[0][3]) == hipSuccess) c->inf_ms[1] += t;
    return QZD_OK;
}

/* runs one of the two marker kernels over d_src[0..n) and leaves the number of positions it found in *cnt and, when they fit
 * the list (cnt <= cap; with `expect`, when there are as many as that), the positions - in no order - at the head of c->h_aux */
typedef void (*marker_kernel_t)(const uint8_t *, uint64_t, uint32_t *, uint32_t, uint32_t *);
static int scan_markers(qzd_ctx *c, marker_kernel_t kernel, const uint8_t *d_src, uint64_t n, uint32_t cap, hipStream_t st, uint32_t *cnt,
                        const uint32_t *expect = NULL)
{
    uint32_t *d_cnt = (uint32_t *)c->d_aux, *d_list = d_cnt + 4;
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, 16, st));
    hipLaunchKernelGGL(kernel, dim3(2048), dim3(256), 0, st, d_src, n, d_list, cap, d_cnt);
    HIPCHK(c, ctl_copy(c->h_aux, d_cnt, 16, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *cnt = *(uint32_t *)c->h_aux;
    if (*cnt == 0 || *cnt > cap || (expect && *cnt != *expect)) return QZD_OK;
    HIPCHK(c, ctl_copy(c->h_aux, d_list, (size_t)*cnt * 4, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return QZD_OK;
}
/* in[0..cnt) sorted into pos: three 11-bit counting passes (the kernel's atomics hand the positions out in no order; a 2 GiB
 * call has 32768 of them; std::sort took over a millisecond between two kernels) */
static void radix_sort3(const uint32_t *in, uint32_t cnt, std::vector<uint32_t> &pos)
{
    std::vector<uint32_t> tmp(cnt);
    pos.resize(cnt);
    for (int pass = 0; pass < 3; pass++) {
        const int sh = 11 * pass;
        uint32_t hist[2049] = {0};
        const uint32_t *src = pass == 0 ? in : pass == 1 ? tmp.data() : pos.data();
        uint32_t *dst = pass == 1 ? pos.data() : tmp.data();
        for (uint32_t i = 0; i < cnt; i++) hist[((src[i] >> sh) & 2047u) + 1]++;
        for (int k = 0; k < 2048; k++) hist[k + 1] += hist[k];
        for (uint32_t i = 0; i < cnt; i++) dst[hist[(src[i] >> sh) & 2047u]++] = src[i];
    }
    pos.swap(tmp);              /* pass 0: in -> tmp, 1: tmp -> pos, 2: pos -> tmp */
}
static int find_markers(qzd_ctx *c, const uint8_t *d_src, uint64_t n, std::vector<uint32_t> &pos, hipStream_t on = NULL)
{
    pos.clear();
    if (n < 4) return QZD_OK;
    uint32_t cap = (uint32_t)(n / 256 + 4096);
    int rc = qzd_aux_reserve(c, (size_t)cap * 4 + 64);
    if (rc) return rc;
    hipStream_t st = on ? on : c->st[0];
    uint32_t cnt = 0;
    rc = scan_markers(c, qzk_marker_kernel, d_src, n, cap - 8, st, &cnt);
    if (rc) return rc;
    if (cnt > cap - 8) return 1;       /* too many candidates: caller falls back to the serial walk */
    if (cnt) radix_sort3((const uint32_t *)c->h_aux, cnt, pos);
    if (getenv("QATZIP_AMD_MARKER_CHECK")) {
        /* the old scan over the same bytes: the same positions, or the call fails (a missed marker would only cost speed -
         * the decode falls back to slower paths - so no parity test would see it) */
        uint32_t rcnt = 0;
        rc = scan_markers(c, qzk_marker_ref_kernel, d_src, n, cap - 8, st, &rcnt, &cnt);
        if (rc) return rc;
        bool same = rcnt == cnt;
        if (same && rcnt) {
            std::vector<uint32_t> ref((const uint32_t *)c->h_aux, (const uint32_t *)c->h_aux + rcnt);
            std::sort(ref.begin(), ref.end());
            same = ref == pos;
        }
        if (!same) { snprintf(c->err, sizeof(c->err), "marker scan: %u positions, the reference scan finds %u or other ones", cnt, rcnt); return QZD_ERR_HIP; }
    }
    return QZD_OK;
}

/* Launch all candidate segments, ordered by compressed size (32-byte classes): lanes (K3b) or waves of one workgroup then
 * carry segments of similar work, which bounds the divergence / tail of mixed data.  Results come back in candidate order. */
static int inflate_grouped(qzd_ctx *c, const uint8_t *d_src, uint8_t *d_dst, std::vector<qzk_infseg> &segs,
                           std::vector<qzk_infres> &res, const std::vector<uint32_t> &start, uint64_t n)
{
    const uint32_t ns = (uint32_t)segs.size();
    std::vector<uint32_t> order(ns);
    order_by_clen(start, n, 5, order);
    std::vector<qzk_infseg> ps(ns);
    std::vector<qzk_infres> pr(ns);
    for (uint32_t i = 0; i < ns; i++) ps[i] = segs[order[i]];
    std::vector<uint32_t> nat;                              /* segs[] is in output order: where each one went */
    if (c->so_host) { nat.resize(ns); for (uint32_t i = 0; i < ns; i++) nat[order[i]] = i; c->so_nat = nat.data(); }
    int rc = qzd_inflate_segments(c, d_src, d_dst, ps.data(), ns, pr.data());
    c->so_nat = NULL;
    if (rc) return rc;
    for (uint32_t i = 0; i < ns; i++) res[order[i]] = pr[i];
    return QZD_OK;
}

static int map_status(int st)
{
    switch (st) {
    case QZK_INF_EOUT: return QZD_ERR_DSTCAP;
    default: return QZD_ERR_DATA;
    }
}

/* The records of a phase A over the first ps.size() candidates of start[], seated largest compressed size first in classes
 * of (1 << shift) bytes: ps[i] is the launch's i-th segment, where[k] = candidate k's place in the launch.  A candidate may
 * read up to `avail` (the member's end, or what has arrived of it); its length hint is the distance to the next start. */
static void build_candidates(const std::vector<uint32_t> &start, uint64_t n, uint32_t avail, uint32_t shift, uint32_t seg_hint,
                             std::vector<qzk_infseg> &ps, std::vector<uint32_t> &where)
{
    const uint32_t ns = (uint32_t)ps.size();
    std::vector<uint32_t> order(ns);
    order_by_clen(start, n, shift, order);
    for (uint32_t i = 0; i < ns; i++) {
        const uint32_t k = order[i];
        where[k] = i;
        ps[i].in_off = start[k]; ps[i].in_len = avail - start[k];
        ps[i].out_off = 0; ps[i].out_cap = seg_hint; ps[i].flags = 0; ps[i].pad = clen(start.data(), (uint32_t)start.size(), n, k);
    }
}
/* the walk's verdict in the records: the links are segments at their output offsets, every other candidate is skipped;
 * chain = the links' places in the launch, in output order */
static void seat_links(const qzp_walk &W, const std::vector<uint32_t> &where, std::vector<qzk_infseg> &ps, std::vector<uint32_t> &chain)
{
    for (qzk_infseg &s : ps) s.flags = QZK_INF_COUNT_ONLY;
    for (const qzp_link &l : W.links) {
        qzk_infseg &s = ps[where[l.cand]];
        s.out_off = l.out_off; s.out_cap = l.out_len; s.flags = 0;
        chain.push_back(where[l.cand]);
    }
}

/* ---- qzd_inflate_stream's paths (the list at the top of this file).  Each answers QZD_PATH_DONE (totals set),
 * QZD_PATH_NEXT (not mine, or the stream is not what I assumed: the next path tries) or an error ---- */
#define QZD_PATH_DONE 1
#define QZD_PATH_NEXT 2
#define QZD_PATH_LANES_NOMEM 3      /* path_lanes: the token scratch could not be had - the wave-per-segment passes need none */
struct inf_lap {                    /* QATZIP_AMD_TRACE=1: wall-clock of the host-side steps on stderr (developer aid) */
    bool on; std::chrono::steady_clock::time_point prev;
    void operator()(const char *what)
    {
        if (!on) return;
        auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[qzd_inflate_stream] %-22s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - prev).count());
        prev = t;
    }
};
struct inf_call {
    qzd_ctx *c; const uint8_t *d_src; uint64_t n; uint8_t *d_dst; uint64_t dst_cap; uint32_t seg_hint;
    uint8_t *h_dst; int *h_sent;
    bool scan_ok; std::vector<uint32_t> start; uint32_t ns;         /* candidate segment starts */
    bool lanes, lanes_nomem;
    std::vector<qzk_infseg> segs; std::vector<qzk_infres> res;     /* (sized when path_lanes is over: it has lists of its own, and 3 MB of zeros are a tenth of a millisecond) */
    uint64_t total_out, total_in;
    inf_lap lap;
};

/* --- 2a. phase A (Huffman decoding into position-independent token streams) runs over every candidate, the host then
 * walks the chain of real segments through the results - a candidate that is no boundary (00 00 FF FF inside compressed
 * data or a stored block) simply drops out - gives each real segment its output offset, and phase B writes only those.
 * One pass whatever the candidates look like. --- */
static int path_lanes(inf_call &S)
{
    qzd_ctx *c = S.c;
    const uint32_t ns = S.ns;
    /* (a lone segment above 16 KB too: sixteen lanes decode 64 KB in 0.50 + 0.45 ms where the wave-per-segment kernel of
     * path 4 takes 1.85 - one thread of 64 KB qzDecompress calls 0.229 -> 0.423 Gbit/s, sixteen threads 3.6 -> 5.1;
     * QATZIP_AMD_LONE_WAVE=1 is the old way) */
    static const bool lone_lanes = getenv("QATZIP_AMD_LONE_WAVE") == NULL;
    if (!(S.scan_ok && S.seg_hint && (ns > 1 || (lone_lanes && S.seg_hint > 16384u)) && S.lanes)) return QZD_PATH_NEXT;
    /* largest compressed size first (256-byte classes, a class in stream order): the segments of a wave carry similar work
     * and the longest start first.  Round 6 measured what it is worth (profiles/r6_phaseA_order.txt; 4 GiB of 64 KB segments):
     * stream order 20.7 ms, classes of 4 KB 15.8 - 16.2, 1 KB 15.2 - 15.4, 256 B 14.9 - 15.3, 32 B 15.4; a wave's duration follows
     * its longest segment's compressed length with a correlation of 0.54.  QATZIP_AMD_INFLATE_CLS=<log2 of the class> */
    static const uint32_t cls_shift = cls_shift_of(getenv("QATZIP_AMD_INFLATE_CLS"));
    std::vector<qzk_infseg> ps(ns);
    std::vector<qzk_infres> pr(ns);
    std::vector<uint32_t> where(ns);                    /* candidate -> its place in the launch */
    build_candidates(S.start, S.n, (uint32_t)S.n, cls_shift, S.seg_hint, ps, where);
    S.lap("segment records");
    HIPCHK(c, hipEventRecord(c->ev[0][0], c->st[0]));
    int rc = two_phase(c, S.d_src, S.d_dst, ps.data(), ns, pr.data(), spec_lanes(ps.data(), ns), c->st[0], false);
    if (rc == QZD_ERR_NOMEM) return QZD_PATH_LANES_NOMEM;
    if (rc) return rc;
    S.lap("phase A");
    const qzp_walk W = chain_walk(S.start.data(), ns, ns, (const qzp_res *)pr.data(), where.data(), 0, 0, S.dst_cap);
    if (!W.ok) return QZD_PATH_NEXT;
    if (W.over < W.links.size()) return QZD_ERR_DSTCAP;             /* (only a chain that is valid as a whole says so) */
    std::vector<uint32_t> chain;                        /* launch indices of the real segments, in output order */
    seat_links(W, where, ps, chain);
    c->so_sent = 0;
    rc = two_phase_resolve(c, S.d_src, S.d_dst, ps.data(), ns, chain.data(), (uint32_t)chain.size(), pr.data(), S.h_dst, c->st[0]);
    if (rc) return rc;
    bool ok = true;
    for (uint32_t i : chain) if (pr[i].status < 0) { ok = false; break; }
    HIPCHK(c, hipEventRecord(c->ev[0][1], c->st[0]));
    HIPCHK(c, hipStreamSynchronize(c->st[0]));
    float t = 0;
    if (hipEventElapsedTime(&t, c->ev[0][0], c->ev[0][1]) == hipSuccess) c->inf_ms[0] += t;
    S.lap("phase B");
    if (!ok) return QZD_PATH_NEXT;
    S.total_out = W.oo; S.total_in = W.total_in;
    if (S.h_sent && S.h_dst && c->so_sent >= S.total_out) *S.h_sent = 1;
    return QZD_PATH_DONE;
}

/* --- 2b. optimistic single pass (QATZIP_AMD_INFLATE=wave, or no token scratch: one wave per segment): candidate k is
 * assumed real and to produce exactly seg_hint bytes at k * seg_hint; validated afterwards --- */
static int path_optimistic(inf_call &S)
{
    qzd_ctx *c = S.c;
    const uint32_t ns = S.ns, seg_hint = S.seg_hint;
    const std::vector<uint32_t> &start = S.start;
    if (!(S.scan_ok && seg_hint && ns > 1 && (!S.lanes || S.lanes_nomem))) return QZD_PATH_NEXT;
    for (uint32_t k = 0; k < ns; k++) {
        uint64_t oo = (uint64_t)k * seg_hint;
        qzk_infseg &s = S.segs[k];
        s.in_off = start[k]; s.in_len = (uint32_t)(S.n - start[k]);
        s.out_off = oo < S.dst_cap ? oo : S.dst_cap;
        s.out_cap = (uint32_t)std::min<uint64_t>(seg_hint, S.dst_cap - s.out_off);
        s.flags = 0;
        s.pad = clen(start.data(), ns, S.n, k);                     /* compressed-length hint for phase A */
    }
    S.lap("segment records");
    c->so_host = S.h_dst; c->so_sent = 0;
    int rc = inflate_grouped(c, S.d_src, S.d_dst, S.segs, S.res, start, S.n);
    c->so_host = NULL;
    if (rc) return rc;
    S.lap("inflate (optimistic)");
    /* consecutive candidates, each exactly seg_hint long, up to the final block */
    for (uint32_t k = 0;; k++) {
        if (k >= ns) return QZD_PATH_NEXT;
        const qzk_infres &r = S.res[k];
        if (r.status == QZK_INF_FINAL) { S.total_out = (uint64_t)k * seg_hint + r.out_len; S.total_in = (uint64_t)start[k] + r.in_used; break; }
        if (r.status != QZK_INF_FLUSH || r.out_len != seg_hint) return QZD_PATH_NEXT;
        if (k + 1 >= ns || start[k + 1] != start[k] + r.in_used) return QZD_PATH_NEXT;
    }
    if (S.h_sent && c->so_sent >= S.total_out) *S.h_sent = 1;       /* every range that holds output went out */
    return QZD_PATH_DONE;
}

/* --- 3. two passes over the candidates: count-only decode of all of them, chain walk + prefix sums on the host, decode
 * of the true segments at exact offsets --- */
static int path_two_pass(inf_call &S)
{
    qzd_ctx *c = S.c;
    const uint32_t ns = S.ns;
    if (!(S.scan_ok && ns > 1)) return QZD_PATH_NEXT;
    for (uint32_t k = 0; k < ns; k++) {
        qzk_infseg &s = S.segs[k];
        s.in_off = S.start[k]; s.in_len = (uint32_t)(S.n - S.start[k]);
        s.out_off = 0; s.out_cap = 0xffffffffu; s.flags = QZK_INF_COUNT_ONLY; s.pad = 0;
    }
    int rc = inflate_grouped(c, S.d_src, S.d_dst, S.segs, S.res, S.start, S.n);
    if (rc) return rc;
    const qzp_walk W = chain_walk(S.start.data(), ns, ns, (const qzp_res *)S.res.data(), NULL, 0, 0, S.dst_cap);
    if (W.over < W.links.size()) return QZD_ERR_DSTCAP;             /* (at the first link that does not fit, whatever follows it) */
    if (!W.ok) return QZD_PATH_NEXT;
    std::vector<qzk_infseg> chain;
    for (const qzp_link &l : W.links) {
        qzk_infseg s = S.segs[l.cand];
        const uint32_t used = S.res[l.cand].in_used;
        s.flags = 0; s.out_off = l.out_off; s.out_cap = l.out_len; s.in_len = used; s.pad = used;
        chain.push_back(s);
    }
    std::vector<qzk_infres> r2(chain.size());
    rc = qzd_inflate_segments(c, S.d_src, S.d_dst, chain.data(), (uint32_t)chain.size(), r2.data());
    if (rc) return rc;
    for (size_t i = 0; i < chain.size(); i++)
        if (r2[i].status < 0 || r2[i].out_len != chain[i].out_cap) return QZD_PATH_NEXT;
    S.total_out = W.oo; S.total_in = W.total_in;
    return QZD_PATH_DONE;
}

/* --- 4. one wave, straight through: streams whose segments reference earlier history or have no markers --- */
static int path_one_wave(inf_call &S)
{
    qzd_ctx *c = S.c;
    qzk_infseg s; qzk_infres r;
    s.in_off = 0; s.in_len = (uint32_t)S.n; s.out_off = 0;
    s.out_cap = (uint32_t)std::min<uint64_t>(S.dst_cap, 0xffffffffu); s.flags = QZK_INF_THROUGH_FLUSH; s.pad = 0;
    int rc = qzd_inflate_segments(c, S.d_src, S.d_dst, &s, 1, &r);
    if (rc) return rc;
    if (r.status != QZK_INF_FINAL) {
        snprintf(c->err, sizeof(c->err), "inflate failed: status %d after %u bytes", r.status, r.out_len);
        return map_status(r.status);
    }
    S.total_out = r.out_len; S.total_in = r.in_used;
    return QZD_PATH_DONE;
}

static int inflate_stream(qzd_ctx *c, const uint8_t *d_src, uint64_t n, uint8_t *d_dst, uint64_t dst_cap,
                          uint32_t seg_hint, uint64_t *h_in_used, uint64_t *h_out_len, uint32_t *h_crc, uint8_t *h_dst, int *h_sent)
{
    if (h_sent) *h_sent = 0;
    if (!c || !d_src || !h_in_used || !h_out_len) return QZD_ERR_PARAM;
    if (n == 0 || n > 0xffffffffull) return QZD_ERR_PARAM;
    hipSetDevice(c->device);
    c->inf_ms[0] = c->inf_ms[1] = c->inf_ms[2] = c->inf_ms[3] = 0;
    *h_in_used = 0; *h_out_len = 0;
    static const bool trace = getenv("QATZIP_AMD_TRACE") != NULL;
    inf_call S;
    S.c = c; S.d_src = d_src; S.n = n; S.d_dst = d_dst; S.dst_cap = dst_cap; S.seg_hint = seg_hint; S.h_dst = h_dst; S.h_sent = h_sent;
    S.total_out = S.total_in = 0;
    S.lap.on = trace; S.lap.prev = std::chrono::steady_clock::now();
    std::vector<uint32_t> mk;
    int rc = find_markers(c, d_src, n, mk);
    S.lap("marker scan + sort");
    if (rc < 0) return rc;
    S.scan_ok = rc == 0;
    S.start.push_back(0);
    if (S.scan_ok) for (uint32_t p : mk) if (p < n) S.start.push_back(p);
    S.ns = (uint32_t)S.start.size();
    const char *force_path = getenv("QATZIP_AMD_INFLATE");
    S.lanes = force_path ? force_path[0] == 'l' : true;            /* every candidate carries a length hint: K lanes per segment at any count */
    S.lanes_nomem = false;
    rc = path_lanes(S);
    if (rc == QZD_PATH_LANES_NOMEM) { S.lanes_nomem = true; rc = QZD_PATH_NEXT; }
    if (rc == QZD_PATH_NEXT) { S.segs.resize(S.ns); S.res.resize(S.ns); rc = path_optimistic(S); }
    if (rc == QZD_PATH_NEXT) rc = path_two_pass(S);
    if (rc == QZD_PATH_NEXT) rc = path_one_wave(S);
    if (rc != QZD_PATH_DONE) return rc;
    *h_in_used = S.total_in; *h_out_len = S.total_out;
    S.lap("chain check / rest");
    if (h_crc) { rc = qzd_crc32(c, d_dst, S.total_out, h_crc); S.lap("crc32"); return rc; }
    return QZD_OK;
}

extern "C" int qzd_inflate_stream(qzd_ctx *c, const uint8_t *d_src, uint64_t n, uint8_t *d_dst, uint64_t dst_cap,
                                  uint32_t seg_hint, uint64_t *h_in_used, uint64_t *h_out_len, uint32_t *h_crc)
{
    return inflate_stream(c, d_src, n, d_dst, dst_cap, seg_hint, h_in_used, h_out_len, h_crc, NULL, NULL);
}

/* the same, for a caller that wants the output in host memory (qzDecompress): when the stream decodes in the first,
 * optimistic pass, its output is sent to h_dst range by range behind the kernels and *h_sent is set; otherwise
 * *h_sent = 0 and the caller copies d_dst out itself */
extern "C" int qzd_inflate_stream_to_host(qzd_ctx *c, const uint8_t *d_src, uint64_t n, uint8_t *d_dst, uint64_t dst_cap,
                                          uint32_t seg_hint, uint64_t *h_in_used, uint64_t *h_out_len, uint32_t *h_crc,
                                          uint8_t *h_dst, int *h_sent)
{
    if (!h_dst || !h_sent) return QZD_ERR_PARAM;
    return inflate_stream(c, d_src, n, d_dst, dst_cap, seg_hint, h_in_used, h_out_len, h_crc, h_dst, h_sent);
}

/* ---- a member that is still in HOST memory: decoded piece by piece while it arrives (round 4) ----
 * qzDecompress used to copy the whole source in, decode, and only then send the output out: for 2 GiB 13 ms of H2D, 12 ms
 * of phase A, and 37 ms of D2H that began when both were over.  Here the compressed bytes are cut into P pieces that go to
 * the device one behind the other; as soon as piece p has landed a helper context (its own streams, scratch and host thread)
 * scans it for flush markers, runs phase A over the candidates that END in the piece, takes the chain's state (next
 * expected segment start, output offset) from piece p - 1, walks its part of the chain, hands the state on, and runs phase
 * B with the output leaving for the host behind it.  So the first output is on its way when an eighth of the input has been
 * decoded, and the link out stays busy while the later pieces' phase A runs.  (The reference keeps its engine fed the same
 * way: requests are submitted while earlier ones are retired, src/qatzip.c:2103-2404.)
 * Anything unusual - too many candidates, a chain that does not close at a piece's end (00 00 FF FF inside compressed data
 * as a piece's last candidate), an error status, a destination too small - abandons the pieces: the input is all on the
 * device by then, and the call goes through inflate_stream() as before, which reports what is wrong.
 * (The cut plan and why the pieces grow: pipe_plan, qzd_inflate_plan.h.) */
struct qzd_pipe {
    std::mutex m; std::condition_variable cv;
    uint32_t P = 0;
    bool issued[QZD_PIPE_MAX] = {};         /* main thread: the piece has landed (the host waits for each copy: a stream made to wait
                                             * for a copy's event was let go only when the copies behind it were over too) */
    bool cand_ok[QZD_PIPE_MAX] = {}; uint32_t lastc[QZD_PIPE_MAX] = {};     /* the last candidate at or before the piece's end */
    bool chain_ok[QZD_PIPE_MAX] = {}; uint32_t nxt[QZD_PIPE_MAX] = {}; uint64_t oo[QZD_PIPE_MAX] = {};   /* the chain after the piece */
    bool final_seen = false; uint64_t total_in = 0, total_out = 0;
    std::mutex m_crc; uint32_t crc[QZD_PIPE_MAX] = {}; uint64_t crc_len[QZD_PIPE_MAX] = {}; bool want_crc = false;      /* CRC-32 of every piece's output, taken while later pieces are still on their way out */
    bool failed = false;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::vector<std::string> log;           /* QATZIP_AMD_TRACE: the pieces' steps, printed when the call is over (printing them
                                             * as they happen moved the helpers' launches: 61.6 ms without the trace, 50.8 with) */

    /* piece p gives up: nobody waits for it any more, and the member goes through as a whole */
    void fail(uint32_t p)
    {
        std::lock_guard<std::mutex> g(m);
        failed = true;
        cand_ok[p] = true; chain_ok[p] = true;
        cv.notify_all();
    }
    /* Each of the next four answers false when the pieces have been abandoned; piece p has then given up as well. */
    /* waits until piece p's bytes are on the device */
    bool wait_landed(uint32_t p)
    {
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, [&] { return issued[p] || failed; });
        if (!failed) return true;
        g.unlock(); fail(p); return false;
    }
    /* piece p's candidates: the last one of the piece before (its segment ends in p) and the markers found behind it, at
     * lo + mk[]; the last of them is handed on in turn */
    bool take_candidates(uint32_t p, uint64_t lo, uint64_t n, const std::vector<uint32_t> &mk, std::vector<uint32_t> &start)
    {
        std::unique_lock<std::mutex> g(m);
        uint32_t prev = 0;
        if (p) { cv.wait(g, [&] { return cand_ok[p - 1]; }); prev = lastc[p - 1]; }
        start.push_back(prev);
        for (uint32_t q : mk) if (lo + q < n && lo + q > prev) start.push_back((uint32_t)(lo + q));
        lastc[p] = start.back(); cand_ok[p] = true;
        cv.notify_all();
        if (!failed) return true;
        g.unlock(); fail(p); return false;
    }
    /* the chain as the piece before left it: the start it expects next, the output offset, whether the final block is behind it */
    bool take_chain(uint32_t p, uint32_t *want, uint64_t *out_off, bool *fin)
    {
        std::unique_lock<std::mutex> g(m);
        *want = 0; *out_off = 0;
        if (p) { cv.wait(g, [&] { return chain_ok[p - 1]; }); *want = nxt[p - 1]; *out_off = oo[p - 1]; }
        *fin = final_seen;
        if (!failed) return true;
        g.unlock(); fail(p); return false;
    }
    /* the chain after piece p, for the next one (ok false: the chain broke here) */
    bool publish_chain(uint32_t p, bool ok, bool fin, uint32_t next, uint64_t out_off, uint64_t t_in)
    {
        std::lock_guard<std::mutex> g(m);
        if (!ok) failed = true;
        nxt[p] = next; oo[p] = out_off; chain_ok[p] = true;
        if (ok && fin && !final_seen) { final_seen = true; total_in = t_in; total_out = out_off; }
        cv.notify_all();
        return !failed;
    }
};

static void pipe_piece_body(qzd_ctx *H, qzd_ctx *c, qzd_pipe *S, uint32_t p, const uint8_t *d_src, uint64_t n, uint8_t *d_dst, uint64_t dst_cap,
                            uint32_t seg_hint, const uint64_t *cut, uint8_t *h_dst)
{
    hipSetDevice(H->device);
    static const bool trace = getenv("QATZIP_AMD_TRACE") != NULL;   /* developer aid: when each step of each piece was over */
    auto lap = [&](const char *what) {
        if (!trace) return;
        char line[160];
        snprintf(line, sizeof(line), "[pipe] piece %u %-18s at %8.3f ms", p, what,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - S->t0).count());
        std::lock_guard<std::mutex> g(S->m);
        S->log.push_back(line);
    };
    hipStream_t st = H->st[0];
    const bool last = p + 1 == S->P;
    if (!S->wait_landed(p)) return;
    /* candidates that end in (cut[p], cut[p + 1]]: the marker's four bytes may begin three bytes before the piece */
    const uint64_t lo = cut[p] >= 3 ? cut[p] - 3 : 0, hi = cut[p + 1];
    std::vector<uint32_t> mk;
    if (find_markers(H, d_src + lo, hi - lo, mk, st) != QZD_OK) { S->fail(p); return; }
    lap("landed, scanned");
    std::vector<uint32_t> start;
    if (!S->take_candidates(p, lo, n, mk, start)) return;
    /* my segments: from every start to the next one; the last start is the next piece's first (the last piece's own, to n) */
    const uint32_t ns = last ? (uint32_t)start.size() : (uint32_t)start.size() - 1;
    std::vector<qzk_infseg> ps(ns);
    std::vector<qzk_infres> pr(ns);
    std::vector<uint32_t> where(ns), chain;
    if (ns) {
        /* largest compressed size first, in 32-byte classes; a candidate reads what has landed - not a byte more */
        build_candidates(start, n, (uint32_t)(last ? n : hi), 5, seg_hint, ps, where);
        lap("phase A begins");
        if (two_phase(H, d_src, d_dst, ps.data(), ns, pr.data(), spec_lanes(ps.data(), ns), st, false) != QZD_OK) { S->fail(p); return; }
        lap("phase A");
    }
    /* the chain through my segments, from where the piece before left it */
    uint32_t want = 0; uint64_t oo0 = 0; bool fin = false;         /* oo0: where my output begins */
    if (!S->take_chain(p, &want, &oo0, &fin)) return;
    qzp_walk W;
    W.ok = true; W.final = false; W.total_in = 0; W.oo = oo0; W.over = 0;
    if (!fin) {
        W = chain_walk(start.data(), (uint32_t)start.size(), ns, (const qzp_res *)pr.data(), where.data(), want, oo0, dst_cap);
        if (W.over < W.links.size()) W.ok = false;                  /* the destination is too small */
        if (W.ok && !W.final && last) W.ok = false;                 /* the stream ends without its final block */
    }
    const uint64_t oo = W.oo;
    if (!S->publish_chain(p, W.ok, fin || W.final, start.back(), oo, W.total_in)) return;
    lap("chain");
    if (W.links.empty()) return;
    H->inf_ms[2] = 0;
    {   /* what phase A of this piece took, for qzd_last_inflate_timing() of the call (the pieces' kernels overlap: a sum of
         * kernel times, not a span) */
        std::lock_guard<std::mutex> g(S->m);
        c->inf_ms[3] += H->inf_ms[3]; c->inf_ms[0] += H->inf_ms[3];
        H->inf_ms[3] = 0;
    }
    seat_links(W, where, ps, chain);
    /* my output's CRC-32 (the caller combines the pieces'), taken on the caller's context - idle while the pieces run - behind
     * my phase B and WHILE my output leaves: one pass over 2 GiB after the last piece had left cost the call 0.7 ms with the
     * link idle */
    uint32_t crc_mine = 0; bool crc_done = false;
    const std::function<void()> crc_fn = [&] {
        std::lock_guard<std::mutex> g(S->m_crc);
        crc_done = hipStreamWaitEvent(c->st[0], H->ev[1][2], 0) == hipSuccess && qzd_crc32(c, d_dst + oo0, oo - oo0, &crc_mine) == QZD_OK;
    };
    if (two_phase_resolve(H, d_src, d_dst, ps.data(), ns, chain.data(), (uint32_t)chain.size(), pr.data(), h_dst, st, c->pq_out,
                          S->want_crc && oo > oo0 ? &crc_fn : NULL) != QZD_OK) { S->fail(p); return; }
    for (uint32_t i : chain) if (pr[i].status < 0) { S->fail(p); return; }
    if (trace) {
        char line[160];
        snprintf(line, sizeof(line), "[pipe] piece %u phase B kernels %.3f ms, %u segments", p, H->inf_ms[2], (uint32_t)chain.size());
        std::lock_guard<std::mutex> g(S->m);
        S->log.push_back(line);
    }
    { std::lock_guard<std::mutex> g(S->m); c->inf_ms[2] += H->inf_ms[2]; c->inf_ms[0] += H->inf_ms[2]; }
    lap("phase B, sent");
    if (crc_done) { std::lock_guard<std::mutex> g(S->m); S->crc[p] = crc_mine; S->crc_len[p] = oo - oo0; }
}
/* a helper thread's entry: nothing may leave it as an exception (std::terminate inside a C API) - a piece that runs out of
 * host memory counts as failed and the member goes through as a whole */
static void pipe_piece(qzd_ctx *H, qzd_ctx *c, qzd_pipe *S, uint32_t p, const uint8_t *d_src, uint64_t n, uint8_t *d_dst, uint64_t dst_cap,
                       uint32_t seg_hint, const uint64_t *cut, uint8_t *h_dst)
{
    try { pipe_piece_body(H, c, S, p, d_src, n, d_dst, dst_cap, seg_hint, cut, h_dst); }
    catch (...) { S->fail(p); }
}

/* d_src: where the n bytes at h_src are to stand on the device (they are all there when this returns, whatever it
 * returns); the rest as qzd_inflate_stream_to_host */
extern "C" int qzd_inflate_stream_from_host(qzd_ctx *c, const uint8_t *h_src, uint64_t n, uint8_t *d_src, uint8_t *d_dst, uint64_t dst_cap,
                                            uint32_t seg_hint, uint64_t *h_in_used, uint64_t *h_out_len, uint32_t *h_crc,
                                            uint8_t *h_dst, int *h_sent)
{
    if (!c || !h_src || !d_src || !h_dst || !h_sent || !h_in_used || !h_out_len) return QZD_ERR_PARAM;
    if (n == 0 || n > 0xffffffffull) return QZD_ERR_PARAM;
    hipSetDevice(c->device);
    *h_sent = 0;
    /* the plan: cut[0] = 0 <= cut[1] <= ... <= cut[P] = n */
    uint64_t cut[QZD_PIPE_MAX + 1];
    uint32_t P = 0;
    pipe_plan(n, cut, &P);
    const char *pe = getenv("QATZIP_AMD_PIPE");                     /* pieces (0 / 1: the whole member at once); equal ones unless QATZIP_AMD_PIPE_CUTS says where */
    if (pe) pipe_plan_equal(n, atoi(pe), cut, &P);
    if (!seg_hint) P = 0;
    if (P >= 2 && qzd_pipe_streams(c) != QZD_OK) { (void)hipGetLastError(); P = 0; }
    for (uint32_t p = 0; p < P; p++) {
        if (!c->pipe_ctx[p] && qzd_create_helper(c->device, &c->pipe_ctx[p]) != QZD_OK) { P = p; break; }
        if (!c->pipe_ev[p] && hipEventCreateWithFlags(&c->pipe_ev[p], hipEventDisableTiming) != hipSuccess) { P = p; break; }
    }
    if (P >= 2) cut[P] = n;                                         /* (fewer helpers than planned: the last one takes the rest) */
    if (P < 2) {
        HIPCHK(c, hipMemcpyAsync(d_src, h_src, n, hipMemcpyHostToDevice, c->st[0])); HIPCHK(c, hipStreamSynchronize(c->st[0]));      /* (not the null stream) */
        return inflate_stream(c, d_src, n, d_dst, dst_cap, seg_hint, h_in_used, h_out_len, h_crc, h_dst, h_sent);
    }
    c->inf_ms[0] = c->inf_ms[1] = c->inf_ms[2] = c->inf_ms[3] = 0;
    qzd_pipe S;
    S.P = P;
    S.want_crc = h_crc != NULL;
    if (const char *ce = getenv("QATZIP_AMD_PIPE_CUTS")) pipe_cuts_percent(n, ce, P, cut);
    pipe_cuts_monotone(cut, P);
    std::vector<std::thread> th;
    th.reserve(P);
    for (uint32_t p = 0; p < P; p++) {
        /* a piece whose thread cannot be started counts as failed (the others must not wait for it), and the call goes
         * through as a whole below - nothing may leave this C entry point as an exception */
        try { th.emplace_back(pipe_piece, c->pipe_ctx[p], c, &S, p, (const uint8_t *)d_src, n, d_dst, dst_cap, seg_hint, (const uint64_t *)cut, h_dst); }
        catch (...) { S.fail(p); }
    }
    /* the copy, two pieces in flight; a piece is the helpers' when the host has seen its copy end.  (A pageable source makes
     * every copy block until it is over: the same, one at a time.) */
    bool copy_ok = true;
    auto landed = [&](uint32_t p) {
        if (copy_ok && hipEventSynchronize(c->pipe_ev[p]) != hipSuccess) copy_ok = false;
        std::lock_guard<std::mutex> g(S.m);
        if (!copy_ok) S.failed = true;
        S.issued[p] = true;
        S.cv.notify_all();
    };
    for (uint32_t p = 0; p < P; p++) {
        if (copy_ok && (hipMemcpyAsync(d_src + cut[p], h_src + cut[p], cut[p + 1] - cut[p], hipMemcpyHostToDevice, c->pq_copy) != hipSuccess ||
                        hipEventRecord(c->pipe_ev[p], c->pq_copy) != hipSuccess)) copy_ok = false;
        if (p) landed(p - 1);
    }
    landed(P - 1);
    for (auto &t : th) t.join();
    for (const std::string &l : S.log) fprintf(stderr, "%s\n", l.c_str());
    HIPCHK(c, hipStreamSynchronize(c->pq_copy));
    if (!copy_ok) {
        snprintf(c->err, sizeof(c->err), "host-to-device copy of a piece failed");
        return QZD_ERR_HIP;
    }
    if (S.failed || !S.final_seen) {
        if (getenv("QATZIP_AMD_TRACE")) fprintf(stderr, "[qzd_inflate_stream_from_host] pieces abandoned, the member goes through as a whole\n");
        return inflate_stream(c, d_src, n, d_dst, dst_cap, seg_hint, h_in_used, h_out_len, h_crc, h_dst, h_sent);
    }
    *h_in_used = S.total_in; *h_out_len = S.total_out; *h_sent = 1;
    if (h_crc) {
        uint32_t crc = 0; uint64_t have = 0;
        for (uint32_t p = 0; p < P; p++)
            if (S.crc_len[p]) { crc = have ? qzd_crc32_combine(crc, S.crc[p], S.crc_len[p]) : S.crc[p]; have += S.crc_len[p]; }
        if (have != S.total_out) return qzd_crc32(c, d_dst, S.total_out, h_crc);     /* (cannot happen: every piece on the chain reports) */
        *h_crc = crc;
    }
    return QZD_OK;
}

#ifdef QZK_SPEC_PROF
extern "C" int qzd_spec_prof(unsigned long long *out, uint32_t nwaves)
{
    static unsigned long long zero[8192][8];
    if (!out) {                                                     /* reset */
        unsigned long long st[8] = {~0ull, 0, ~0ull, 0, ~0ull, 0, ~0ull, 0};
        hipMemcpyToSymbol(HIP_SYMBOL(qzk_stamp), st, sizeof(st), 0, hipMemcpyHostToDevice);
        hipMemcpyToSymbol(HIP_SYMBOL(qzk_stamp_b), st, 16, 0, hipMemcpyHostToDevice);
        return hipMemcpyToSymbol(HIP_SYMBOL(qzk_spec_prof), zero, sizeof(zero), 0, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
    }
    if (nwaves == 0xffffffffu) {
        hipMemcpyFromSymbol(out, HIP_SYMBOL(qzk_stamp), 64, 0, hipMemcpyDeviceToHost);
        return hipMemcpyFromSymbol(out + 4, HIP_SYMBOL(qzk_stamp_b), 16, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
    }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(qzk_spec_prof), (size_t)(nwaves < 8192 ? nwaves : 8192) * 64, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

#ifdef QZK_SPEC_PROF
extern __device__ unsigned int qzk_spec_seg[1 << 17];
/* profiling builds: the per-segment clocks of the last phase A (launch order), n <= 131072 */
extern "C" int qzd_spec_seg_prof(unsigned int *out, uint32_t n)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(qzk_spec_seg), (size_t)(n < (1u << 17) ? n : (1u << 17)) * 4, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

/* developer aid: resident workgroups per CU the runtime grants phase A's kernels */
extern "C" int qzd_inflate_occupancy(int out[4])
{
    int a = -1, b = -1, c4 = -1, d = -1;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, qzk_inflate_tok_kernel<16, QZD_TOK_OCC>, 16, 0);
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, qzk_inflate_spec_kernel<4, 2>, 64, 0);
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&c4, qzk_inflate_spec_kernel<8, 3>, 64, 0);
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&d, qzk_lz_resolve_kernel, 64 * QZK_RES_WAVES, 0);
    out[0] = a; out[1] = b; out[2] = c4; out[3] = d;
    return 0;
}

extern "C" uint64_t qzd_inflate_scratch_bytes(qzd_ctx *c) { return c ? (uint64_t)c->big_cap : 0; }

extern "C" int qzd_last_inflate_timing(qzd_ctx *c, float ms[4])
{
    if (!c || !ms) return QZD_ERR_PARAM;
    ms[0] = c->inf_ms[0]; ms[1] = c->inf_ms[1]; ms[2] = c->inf_ms[2]; ms[3] = c->inf_ms[3];
    return QZD_OK;
}
