/* qzd_slot_host.h — host arithmetic of the wave-per-chunk compressors (qzd_device.hip: slot_rounds), plain C++ for the CPU test */
#ifndef QZD_SLOT_HOST_H
#define QZD_SLOT_HOST_H
#include <stdint.h>

#define QZD_SLOT_ROUND 16384u           /* slots per round at most */
#define QZD_SLOT_GIGABYTE (1ull << 30)  /* the budget of every path whose slots can be large */

/* slots per round for `items` chunks whose slots are `stride` bytes apart: QZD_SLOT_ROUND at most, and where a budget is
 * given (0 = none) no more than fit into it, though always one */
static inline uint32_t qzd_slot_batch(uint32_t items, uint32_t stride, uint64_t budget)
{
    const uint32_t batch = items < QZD_SLOT_ROUND ? items : QZD_SLOT_ROUND;
    if (!budget || (uint64_t)batch * stride <= budget) return batch;
    return budget / stride ? (uint32_t)(budget / stride) : 1u;
}

/* LZ4 frames: no budget for one-block frames (16384 slots of 65632 bytes are just above a gigabyte, and stay) */
static inline uint64_t qzd_lz4_slot_budget(uint32_t frame_sz) { return frame_sz > 65536 ? QZD_SLOT_GIGABYTE : 0; }

/* LZ4F_compressFrameBound of ONE frame of n bytes in linked 64 KB blocks: header, a word per block, the bytes, end mark, checksum */
static inline uint64_t qzd_lz4_linked_bound(uint64_t n) { return 19 + 4 * ((n + 65535) >> 16) + n + 8; }
#endif
