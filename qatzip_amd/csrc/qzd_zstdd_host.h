/*
 * qzd_zstdd_host.h — the host side of the zstd decoder (qzd_zstdd.hip: qzd_zstd_decompress_frames; qz_api.cpp: a zstd
 * decode session; the qzstd-amd tool): a frame's extent from its header and its block headers, the scratch a frame needs,
 * the rounds a call's frames are taken in.  Plain C++ without a HIP call, so that the emulator driver
 * (tests/sim/sim_zstdd.cpp) runs these very lines, on their own under a sanitizer too.  The extent is plain C as well (the
 * tool); the scratch plan needs the kernels' records: include behind qzk_zstdd.h for it.
 */
#ifndef QZD_ZSTDD_HOST_H
#define QZD_ZSTDD_HOST_H
#include <stdint.h>
#include <string.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#define QZD_ZD_TRUNCATED (-3)       /* the input ends inside the frame */
#define QZD_ZD_MALFORMED (-1)       /* no zstd or skippable magic, the reserved descriptor bit, block type 3 */

/* the scratch of one round of frames stays under this many bytes (a frame that needs more is a round of its own): 2 GiB
 * holds about 4800 frames of 64 KB, more than the 3072 that stage E keeps in flight on 256 CUs - with 256 MiB a round was 150
 * waves on 256 CUs and the call ran at a quarter of the rate (profiles/zstd_decode_rates.txt) */
#define QZD_ZD_SCRATCH_CAP (2048ull << 20)

/* Walks the frame at p[0 .. n): the frame header and the 3-byte block headers, nothing inside a block.  Returns the frame's
 * length, checksum included, or QZD_ZD_TRUNCATED / QZD_ZD_MALFORMED.  *has_content / *content: Frame_Content_Size;
 * *bound: what the blocks can produce - exact for Raw and RLE blocks, min(window, 128 KB) for a Compressed one - so that a
 * frame without a content size still gets an out_cap.  A skippable frame (magic 0x184D2A50 - 5F) has an extent, a content
 * size of 0 and produces nothing.  *nblocks (optional): the frame's blocks. */
static inline int64_t qzd_zd_frame_walk(const uint8_t *p, uint64_t n, uint64_t *content, bool *has_content, uint64_t *bound, uint32_t *nblocks)
{
    *content = 0; *has_content = false; *bound = 0;
    if (nblocks) *nblocks = 0;
    if (n < 4) return QZD_ZD_TRUNCATED;
    const uint32_t magic = p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    if ((magic & 0xfffffff0u) == 0x184D2A50u) {
        if (n < 8) return QZD_ZD_TRUNCATED;
        const uint64_t sz = p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24;
        if (sz > n - 8) return QZD_ZD_TRUNCATED;
        *has_content = true;
        return (int64_t)(8 + sz);
    }
    if (magic != 0xFD2FB528u) return QZD_ZD_MALFORMED;
    if (n < 5) return QZD_ZD_TRUNCATED;
    const uint32_t fhd = p[4];
    if (fhd & 0x08) return QZD_ZD_MALFORMED;
    const uint32_t single = (fhd >> 5) & 1, flag = fhd >> 6, did = fhd & 3;
    const uint32_t fb = flag == 0 ? single : flag == 1 ? 2u : flag == 2 ? 4u : 8u;
    const uint32_t db = did == 3 ? 4u : did;
    uint64_t pos = 5 + (single ? 0u : 1u) + db + fb;
    if (n < pos) return QZD_ZD_TRUNCATED;
    uint64_t window = 0;
    if (!single) {
        const uint32_t wlog = 10 + (p[5] >> 3);
        window = (1ull << wlog) + ((1ull << wlog) >> 3) * (p[5] & 7u);
    }
    uint64_t c = 0;
    for (uint32_t i = 0; i < fb; i++) c |= (uint64_t)p[pos - fb + i] << (8 * i);
    if (fb == 2) c += 256;
    if (single) window = c;
    *has_content = fb != 0; *content = c;
    const uint64_t bmax = window < 131072 ? window : 131072;
    uint64_t b = 0;
    for (;;) {
        if (n - pos < 3) return QZD_ZD_TRUNCATED;
        const uint32_t bh = p[pos] | (uint32_t)p[pos + 1] << 8 | (uint32_t)p[pos + 2] << 16;
        pos += 3;
        const uint32_t type = (bh >> 1) & 3, bsz = bh >> 3;
        if (type == 3) return QZD_ZD_MALFORMED;
        const uint64_t in = type == 1 ? 1 : bsz;
        if (n - pos < in) return QZD_ZD_TRUNCATED;
        pos += in;
        b += type == 2 ? bmax : bsz;
        if (nblocks) (*nblocks)++;
        if (bh & 1) break;
    }
    if (fhd & 4) { if (n - pos < 4) return QZD_ZD_TRUNCATED; pos += 4; }
    *bound = b;
    return (int64_t)pos;
}
static inline int64_t qzd_zd_frame_extent(const uint8_t *p, uint64_t n, uint64_t *content, bool *has_content, uint64_t *bound)
{
    return qzd_zd_frame_walk(p, n, content, has_content, bound, 0);
}

#ifdef QZK_ZSTDD_H
/* The scratch plan of one frame, from its segment alone (the input is on the device, its block headers are not read here):
 * the literals are at most what the frame produces, <= out_cap; a sequence produces three bytes at least and every block
 * adds one record (its trailing literals, a Raw block, an RLE block) and takes three bytes of input at least:
 * records <= out_cap / 3 + in_len / 3 + 1.  12 bytes a record: about 5 bytes per byte of out_cap and 4 per byte of input. */
static inline void qzd_zd_caps(uint32_t in_len, uint32_t out_cap, uint32_t *lit_cap, uint32_t *rec_cap)
{
    *lit_cap = out_cap;
    *rec_cap = out_cap / 3 + in_len / 3 + 1;
}
/* the literals in a region of whole 16-byte rows with a row to spare (the copy engine loads its literal rows whole), the
 * records behind them */
static inline uint64_t qzd_zd_frame_scratch(uint32_t lit_cap, uint32_t rec_cap)
{
    return (((uint64_t)lit_cap + 15) & ~15ull) + 16 + (((uint64_t)rec_cap * 12 + 15) & ~15ull);
}

/* One round: the frames from `first` on whose scratch stays under `cap` together, one frame at least.  plan[0 .. count)
 * <- their regions; *bytes <- the scratch of the round (16 bytes in front of the first region and behind the last).
 * Returns count. */
static inline uint32_t qzd_zd_round(const qzk_zdseg *segs, uint32_t first, uint32_t nsegs, uint64_t cap, qzk_zdplan *plan, uint64_t *bytes)
{
    uint64_t off = 16;
    uint32_t k = 0;
    for (uint32_t i = first; i < nsegs; i++, k++) {
        uint32_t lc, rc;
        qzd_zd_caps(segs[i].in_len, segs[i].out_cap, &lc, &rc);
        const uint64_t need = qzd_zd_frame_scratch(lc, rc);
        if (k && off + need + 16 > cap) break;
        plan[k].lit_off = off; plan[k].lit_cap = lc;
        plan[k].rec_off = off + (((uint64_t)lc + 15) & ~15ull) + 16; plan[k].rec_cap = rc;
        off += need;
    }
    *bytes = off + 16;
    return k;
}
#endif

#ifdef QZK_ZSTDD_BLOCKS_H
/* The block route (qzk_zstdd_blocks.h).  A frame whose block count the caller knows can have its blocks' bit streams read
 * in parallel.  route: 0 auto - frames of QZD_ZD_BLOCKS_MIN blocks and more, the smallest count at which the route was not
 * slower than stage E (profiles/zstd_decode_blocks.txt: 512 frames a call, 1.03 of stage E's time at one block a frame, 0.87
 * at two, 0.50 at four) -, 1 no frame, 2 every frame whose count is known. */
#define QZD_ZD_BLOCKS_MIN 2u
static inline bool qzd_zdb_routed(int route, uint32_t nblocks)
{
    return route != 1 && nblocks != 0 && (route == 2 || nblocks >= QZD_ZD_BLOCKS_MIN);
}
/* The routed frames among the k frames of a round that starts at segment `first` (h_nblocks may be NULL: none).  fr[0 ..
 * count) <- {segment of the round, hint, first descriptor}; *nblocks <- the round's descriptors, which lie behind the
 * round's scratch (qzd_zd_round).  A block takes three bytes of input at least, so a hint above in_len / 3 is wrong
 * whatever the frame holds: it is cut to in_len / 3 + 1, which is wrong too and keeps the descriptors within what the
 * input could need.  Returns count. */
static inline uint32_t qzd_zdb_round(const qzk_zdseg *segs, const uint32_t *h_nblocks, uint32_t first, uint32_t k, int route,
                                     qzk_zdb_frame *fr, uint64_t *nblocks)
{
    uint32_t n = 0;
    uint64_t nb = 0;
    for (uint32_t i = 0; h_nblocks && i < k; i++) {
        uint32_t hint = h_nblocks[first + i];
        if (!qzd_zdb_routed(route, hint)) continue;
        if (hint > segs[first + i].in_len / 3) hint = segs[first + i].in_len / 3 + 1;
        qzk_zdb_frame f;
        memset(&f, 0, sizeof f);
        f.seg = i; f.hint = hint; f.first_blk = (uint32_t)nb;
        fr[n++] = f;
        nb += hint;
    }
    *nblocks = nb;
    return n;
}
static inline uint64_t qzd_zdb_desc_bytes(uint64_t nblocks) { return nblocks * sizeof(qzk_zdb_desc) + 16; }
#endif

#endif
