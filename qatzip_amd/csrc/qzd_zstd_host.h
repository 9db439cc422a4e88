/*
 * qzd_zstd_host.h — the host side of the zstd calls (qzd_device.hip: qzd_zstd_bound, qzd_zstd_compress_frames,
 * qzd_zstd_encode_frames): the bound, the parameter check, the slot stride, the frame descriptions a caller of
 * qzd_zstd_encode_frames hands over, the scan over frame lengths.  Plain C++ without a HIP call, so that the emulator driver
 * (tests/sim/sim_zstd.cpp) runs these very lines, on their own under a sanitizer too.  Include behind qzk_zstd.h.
 */
#ifndef QZD_ZSTD_HOST_H
#define QZD_ZSTD_HOST_H
#include <stdint.h>

/* what the frames of n bytes in chunks of block_sz can grow to: per chunk of c bytes the Raw block, 4 + 1 + 4 + 3 + c */
static inline uint64_t qzd_zs_bound(uint64_t n, uint32_t block_sz)
{
    if (!block_sz) return 0;
    const uint64_t full = n / block_sz, rest = n % block_sz;
    return full * QZK_ZS_BOUND(block_sz) + (rest ? QZK_ZS_BOUND((uint32_t)rest) : 0);
}

/* hw_buff_sz a power of two in 1 KB .. 128 KB, mini_match 3 or 4 */
static inline bool qzd_zs_params_ok(uint32_t block_sz, uint32_t mini_match)
{
    return mini_match >= 3 && mini_match <= 4 && block_sz >= QZK_L4S_MINBLK && block_sz <= QZK_ZS_MAXBLK && !(block_sz & (block_sz - 1));
}

/* a slot for a frame of up to c bytes: the bound, what the stage may touch behind it, to 16 bytes */
static inline uint32_t qzd_zs_stride(uint32_t c) { return (QZK_ZS_BOUND(c) + QZK_ZS_SLACK + 15u) & ~15u; }

/* h_desc = nframes x (content size, records, literals) -> the kernel's descriptions, records and literals back to back in
 * frame order; *maxc = the largest content size, *nseq / *nlit (optional) = the totals.  false: a content size of 0 or above
 * 128 KB, more literals than content, more records than a third of the content (a record covers three bytes at least). */
static inline bool qzd_zs_describe(const uint32_t *h_desc, uint32_t nframes, qzk_zs_fdesc *fd, uint32_t *maxc, uint64_t *nseq, uint64_t *nlit)
{
    uint64_t s = 0, l = 0;
    *maxc = 0;
    for (uint32_t i = 0; i < nframes; i++) {
        const uint32_t content = h_desc[3 * (size_t)i], ns = h_desc[3 * (size_t)i + 1], nl = h_desc[3 * (size_t)i + 2];
        if (content == 0 || content > QZK_ZS_MAXBLK || nl > content || ns > (content - nl) / 3) return false;
        fd[i].lit0 = l; fd[i].seq0 = s; fd[i].content = content; fd[i].nseq = ns; fd[i].nlit = nl; fd[i].pad = 0;
        s += ns; l += nl;
        if (content > *maxc) *maxc = content;
    }
    if (nseq) *nseq = s;
    if (nlit) *nlit = l;
    return true;
}

/* seq_flags of the _ex calls: the two bits of include/qzamd_zstd_seq.h */
static inline bool qzd_zs_seq_flags_ok(uint32_t flags) { return flags <= (QZK_ZS_SEQ_FSE | QZK_ZS_SEQ_REP); }

/* the words of offset values a wave of qzk_zstd_encode_seq_kernel needs: the records of the longest frame */
static inline uint32_t qzd_zs_ofv_words(const qzk_zs_fdesc *fd, uint32_t nframes)
{
    uint32_t m = 1;
    for (uint32_t i = 0; i < nframes; i++) if (fd[i].nseq > m) m = fd[i].nseq;
    return (m + 3u) & ~3u;
}

/* offs[i] = where frame i begins; returns the total */
static inline uint64_t qzd_zs_scan(const uint32_t *lens, uint32_t n, uint64_t *offs)
{
    uint64_t run = 0;
    for (uint32_t i = 0; i < n; i++) { offs[i] = run; run += lens[i]; }
    return run;
}

#endif
