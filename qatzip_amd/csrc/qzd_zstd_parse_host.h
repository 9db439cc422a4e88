/*
 * qzd_zstd_parse_host.h — the host side of qzd_zstd_compress_frames_parse (qzd_device.hip): what a depth may be, and the plan
 * of a call's rounds - how many chunks a round holds and what each of them takes of the context's scratch.  Plain C++
 * without a HIP call, so that the emulator driver (tests/sim/sim_zstd_parse.cpp) runs these very lines, on their own under a
 * sanitizer too.  Include behind qzk_zstd_parse.h, qzd_zstd_host.h and qzd_slot_host.h.
 */
#ifndef QZD_ZSTD_PARSE_HOST_H
#define QZD_ZSTD_PARSE_HOST_H
#include <stdint.h>

#define QZD_ZP_ROUND 4096u              /* chunks per round at most: a wave each, sixteen a CU */
#define QZD_ZP_BUDGET (4ull << 30)      /* of a round's scratch and slots together */

/* 0: the parse of K4s; 1 .. 256: the search attempts per position */
static inline bool qzd_zp_depth_ok(uint32_t depth) { return depth <= QZK_ZP_MAXDEPTH; }

/* a round of a call over nchunks chunks of block_sz (qzd_zs_params_ok) bytes: `batch` chunks, each with chunk_b bytes of
 * scratch (head_b of them the head table, which the round zeroes) and a slot of `stride` bytes */
typedef struct { uint32_t batch, stride; uint64_t chunk_b, head_b; } qzd_zp_plan;
static inline qzd_zp_plan qzd_zp_plan_for(uint32_t block_sz, uint32_t nchunks)
{
    qzd_zp_plan P;
    P.stride = qzd_zs_stride(block_sz);
    P.chunk_b = QZK_ZP_CHUNKB(block_sz);
    P.head_b = QZK_ZP_HEADB(block_sz);
    /* (a chunk's scratch and slot stay far below 4 GiB: 19 bytes per byte of a chunk of 128 KB at most) */
    P.batch = qzd_slot_batch(nchunks < QZD_ZP_ROUND ? nchunks : QZD_ZP_ROUND, (uint32_t)(P.chunk_b + P.stride), QZD_ZP_BUDGET);
    return P;
}

#endif
