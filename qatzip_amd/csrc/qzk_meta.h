/*
 * qzk_meta.h — K10-K12: the kernels of block-addressable compression (qzCompressWithMetadataExt and its relatives,
 * include/qatzip.h) for gfx950.
 *
 *   K10 qzk_crcn_kernel          CRC of many byte ranges under a Rocksoft-model config of width 32 or 64, a workgroup a range
 *   K11 qzk_xxh32_ranges_kernel  XXH32 (seed 0) of many ranges, a wave a range
 *   K12 qzk_blocks_plan_kernel   per block: compressed stream or plaintext (comp_thrshold), exclusive scan of the chosen
 *       qzk_blocks_pack_kernel   sizes, gather into the destination, 16 bytes per lane
 *       qzk_blocks_unpack_kernel stored blocks of a decompress call to their places
 *
 * K10 has ONE data path for every config: the register is kept left-aligned in 64 bits and runs MSB-first (the "normal"
 * form); reflect_in is a bit-reverse of every input byte and reflect_out a bit-reverse of the final register.  A width-32
 * polynomial therefore lives in bits 63..32 and the low half stays zero.  Shape as qzk_block_crc32 (qzk_deflate_huff.h):
 * the workgroup builds the byte table of the polynomial in LDS, every thread runs a contiguous slice from register 0 (the
 * thread that owns the range's first byte from the range's starting register), the slices are shifted by x^(8*tail) mod P
 * and XOR-reduced - crc_combine algebra, no serial pass.
 */
#ifndef QZK_META_H
#define QZK_META_H
#include "qzk_common.h"
#include "qzk_lz4.h"

#ifdef QZ_SIM
#define QZ_HD static inline
#else
#define QZ_HD static __host__ __device__ __forceinline__
#endif

#define QZK_CRCN_T 256             /* threads per workgroup of K10 */

typedef struct { uint64_t off; uint32_t len; uint32_t pad; } qzk_mrange;

/* a CRC config as the kernel wants it: polynomial and initial register left-aligned in 64 bits */
typedef struct { uint64_t poly, init, xor_out; uint32_t width, refin, refout, pad; } qzk_crcn_cfg;

QZ_HD uint64_t qzk_brev64(uint64_t v)
{
    v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    v = ((v >> 4) & 0x0f0f0f0f0f0f0f0full) | ((v & 0x0f0f0f0f0f0f0f0full) << 4);
    v = ((v >> 8) & 0x00ff00ff00ff00ffull) | ((v & 0x00ff00ff00ff00ffull) << 8);
    v = ((v >> 16) & 0x0000ffff0000ffffull) | ((v & 0x0000ffff0000ffffull) << 16);
    return (v >> 32) | (v << 32);
}
QZ_HD uint32_t qzk_brev8(uint32_t b)
{
    b = ((b >> 1) & 0x55u) | ((b & 0x55u) << 1);
    b = ((b >> 2) & 0x33u) | ((b & 0x33u) << 2);
    return ((b >> 4) & 0x0fu) | ((b & 0x0fu) << 4);
}

QZ_HD qzk_crcn_cfg qzk_crcn_make(uint32_t width, uint64_t polynomial, uint64_t initial_value, uint32_t reflect_in,
                                 uint32_t reflect_out, uint64_t xor_out)
{
    qzk_crcn_cfg c;
    const uint32_t sh = 64 - width;
    c.poly = polynomial << sh; c.init = initial_value << sh;
    c.xor_out = width == 64 ? xor_out : (xor_out & 0xffffffffull);
    c.width = width; c.refin = reflect_in; c.refout = reflect_out; c.pad = 0;
    return c;
}
/* left-aligned register -> the CRC a caller sees, and back (a finalised CRC is what chains from call to call) */
QZ_HD uint64_t qzk_crcn_final(const qzk_crcn_cfg &c, uint64_t reg)
{
    uint64_t v = c.refout ? qzk_brev64(reg) : reg >> (64 - c.width);      /* the reversed register is right-aligned already */
    return v ^ c.xor_out;
}
QZ_HD uint64_t qzk_crcn_unfinal(const qzk_crcn_cfg &c, uint64_t crc)
{
    const uint64_t v = crc ^ c.xor_out;
    return c.refout ? qzk_brev64(v) : v << (64 - c.width);
}

/* a(x) * x mod P and a(x) * b(x) mod P; polynomials of degree < width, the coefficient of x^(width-1) in bit 63 */
QZ_DEV uint64_t qzk_crcn_mulx(uint64_t a, uint64_t P) { return (a << 1) ^ ((a >> 63) ? P : 0ull); }
QZ_DEV uint64_t qzk_crcn_mulmod(uint64_t a, uint64_t b, uint64_t P, uint32_t width)
{
    uint64_t r = 0;
    for (uint32_t i = 0; i < width; i++) {                          /* Horner over b, highest coefficient first */
        r = qzk_crcn_mulx(r, P);
        if ((b >> (63 - i)) & 1) r ^= a;
    }
    return r;
}

struct qzk_crcn_lds {
    uint64_t tab[256];             /* tab[b] = b(x) * x^width mod P: one byte step of the register */
    uint64_t x2n[36];              /* x^(8 * 2^k) mod P */
    uint64_t red[QZK_CRCN_T / 64];
};

/* x^(8 * bytes) mod P from the table of squares */
QZ_DEV uint64_t qzk_crcn_xpow(const qzk_crcn_lds *S, uint64_t bytes, uint64_t P, uint32_t width)
{
    uint64_t r = 0; bool have = false;
    for (int k = 0; bytes; k++, bytes >>= 1) {
        if (!(bytes & 1)) continue;
        r = have ? qzk_crcn_mulmod(r, S->x2n[k], P, width) : S->x2n[k];
        have = true;
    }
    return r;                                                       /* (bytes == 0 is the caller's case) */
}

/* the register after p[0..n) from `reg` */
QZ_DEV uint64_t qzk_crcn_run(const qzk_crcn_lds *S, const uint8_t *p, uint32_t n, uint64_t reg, uint32_t refin)
{
    uint32_t i = 0;
    for (; i + 4 <= n; i += 4) {
        uint32_t w = qz_ld32(p + i);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t b = w & 0xff; w >>= 8;
            if (refin) b = qzk_brev8(b);
            reg = S->tab[(uint32_t)(reg >> 56) ^ b] ^ (reg << 8);
        }
    }
    for (; i < n; i++) {
        uint32_t b = p[i];
        if (refin) b = qzk_brev8(b);
        reg = S->tab[(uint32_t)(reg >> 56) ^ b] ^ (reg << 8);
    }
    return reg;
}

/* crc_out[r] = CRC (finalised, right-aligned) of data[ranges[r]) under cfg, continuing from start[r] - the finalised CRC of
 * the bytes before the range - or, with start == NULL, from the empty message.  QZK_CRCN_T threads, a workgroup a range. */
QZ_KERNEL_MAX(QZK_CRCN_T) qzk_crcn_kernel(const uint8_t *data, const qzk_mrange *ranges, uint32_t nranges, qzk_crcn_cfg cfg,
                                          const uint64_t *start, uint64_t *crc_out)
{
    QZ_LDS qzk_crcn_lds S;
    const uint32_t r = blockIdx.x, t = threadIdx.x;
    if (r >= nranges) return;
    const int lane = (int)(t & 63), wv = (int)(t >> 6);
    const uint64_t P = cfg.poly; const uint32_t W = cfg.width;
    {
        uint64_t c = (uint64_t)t << 56;
        for (int k = 0; k < 8; k++) c = qzk_crcn_mulx(c, P);
        S.tab[t] = c;
    }
    const uint8_t *p = data + ranges[r].off;
    const uint32_t n = ranges[r].len;
    const uint32_t slice = (n + QZK_CRCN_T - 1) / QZK_CRCN_T;
    if (t == 0) {
        /* x^8 = the unit (bit 64 - width) times x, eight times; then squares as far as the largest tail needs them */
        uint64_t v = 1ull << (64 - W);
        for (int k = 0; k < 8; k++) v = qzk_crcn_mulx(v, P);
        S.x2n[0] = v;
        for (int k = 1; k < 36 && ((uint64_t)n >> k); k++) S.x2n[k] = v = qzk_crcn_mulmod(v, v, P, W);
    }
    qz_block_sync();
    const uint32_t b0 = t * slice < n ? t * slice : n, b1 = (t + 1) * slice < n ? (t + 1) * slice : n;
    uint64_t reg = t == 0 ? (start ? qzk_crcn_unfinal(cfg, start[r]) : cfg.init) : 0ull;
    reg = qzk_crcn_run(&S, p + b0, b1 - b0, reg, cfg.refin);
    const uint32_t tail = n - b1;
    uint64_t part = (reg && tail) ? qzk_crcn_mulmod(reg, qzk_crcn_xpow(&S, tail, P, W), P, W) : reg;
    uint32_t lo = (uint32_t)part, hi = (uint32_t)(part >> 32);
    for (int d = 32; d >= 1; d >>= 1) { lo ^= qz_shfl(lo, lane ^ d); hi ^= qz_shfl(hi, lane ^ d); }
    if (lane == 0) S.red[wv] = (uint64_t)hi << 32 | lo;
    qz_block_sync();
    if (t == 0) {
        uint64_t v = 0;
        for (int k = 0; k < QZK_CRCN_T / 64; k++) v ^= S.red[k];
        crc_out[r] = qzk_crcn_final(cfg, v);
    }
}

/* ------------------------------------------------------------------ K11: XXH32 of ranges */
QZ_KERNEL_MAX(64) qzk_xxh32_ranges_kernel(const uint8_t *data, const qzk_mrange *ranges, uint32_t nranges, uint32_t *hash_out)
{
    QZ_LDS __attribute__((aligned(16))) uint8_t stage[2048];        /* qzk_wave_xxh32_staged's stripes */
    const uint32_t r = blockIdx.x;
    if (r >= nranges) return;
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t h = qzk_wave_xxh32_staged(data + ranges[r].off, ranges[r].len, stage, lane);
    if (lane == 0) hash_out[r] = h;
}

/* ------------------------------------------------------------------ K12: block pack / unpack */
#define QZK_PLAN_T 1024            /* one workgroup scans every block of a call, QZK_PLAN_T a step */

/* what the pack step decides for a block: where it goes, how many bytes, compressed (1) or stored (0); from = where its
 * bytes are taken from (the slot streams, or the plaintext) */
typedef struct { uint64_t offset; uint32_t size, flags; } qzk_blockpos;

/* Block k of the n input bytes cut every block_sz: its stream is slot_len[k] bytes, the streams stand back to back (an
 * exclusive scan of slot_len finds them).  It is kept when slot_len[k] <= thrshold, otherwise the plaintext is stored.
 * pos[k] / from[k] as above, in_rng[k] the plaintext, out_rng[k] the block in the destination (empty when it does not
 * fit dst_cap: such a block is not written); total[0] = bytes of all blocks. */
QZ_KERNEL_MAX(QZK_PLAN_T) qzk_blocks_plan_kernel(const uint32_t *slot_len, uint32_t nblocks, uint64_t n, uint32_t block_sz,
                                                 uint32_t thrshold, uint64_t dst_cap, qzk_blockpos *pos, uint64_t *from,
                                                 qzk_mrange *in_rng, qzk_mrange *out_rng, uint64_t *total)
{
    QZ_LDS uint32_t wa[QZK_PLAN_T / 64], wc[QZK_PLAN_T / 64];
    const uint32_t t = threadIdx.x;
    const int lane = (int)(t & 63), wv = (int)(t >> 6);
    uint64_t carry_a = 0, carry_c = 0;                              /* streams / chosen bytes before this step (uniform) */
    for (uint32_t base = 0; base < nblocks; base += QZK_PLAN_T) {
        const uint32_t k = base + t;
        const bool live = k < nblocks;
        const uint64_t poff = (uint64_t)k * block_sz;
        const uint32_t plain = live ? (uint32_t)(n - poff < block_sz ? n - poff : block_sz) : 0;
        const uint32_t a = live ? slot_len[k] : 0;
        const uint32_t keep = live && a <= thrshold;
        const uint32_t c = keep ? a : plain;
        const uint32_t ia = qz_wave_incl_scan(a), ic = qz_wave_incl_scan(c);
        if (lane == 63) { wa[wv] = ia; wc[wv] = ic; }
        qz_block_sync();
        uint64_t pa = carry_a, pc = carry_c, ta = 0, tc = 0;
        for (int w = 0; w < QZK_PLAN_T / 64; w++) {
            if (w < wv) { pa += wa[w]; pc += wc[w]; }
            ta += wa[w]; tc += wc[w];
        }
        if (live) {
            const uint64_t off = pc + ic - c;
            pos[k].offset = off; pos[k].size = c; pos[k].flags = keep;
            from[k] = keep ? pa + ia - a : poff;
            in_rng[k].off = poff; in_rng[k].len = plain; in_rng[k].pad = 0;
            out_rng[k].off = off; out_rng[k].len = off + c <= dst_cap ? c : 0; out_rng[k].pad = 0;
        }
        carry_a += ta; carry_c += tc;
        qz_block_sync();                                            /* wa / wc are rewritten by the next step */
    }
    if (t == 0) total[0] = carry_c;
}

typedef struct __attribute__((packed, aligned(1))) { uint32_t v[4]; } qz_u128u;
typedef struct __attribute__((aligned(16))) { uint32_t v[4]; } qz_u128a;

/* dst[0..n) = src[0..n) by a 256-thread workgroup: bytes up to dst's 16-byte boundary, then 16 bytes per lane (the
 * source at whatever alignment it has), then the last bytes */
QZ_DEV void qzk_block_copy16(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t t)
{
    uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
    if (head > n) head = n;
    if (t < head) dst[t] = src[t];
    const uint32_t n16 = (n - head) >> 4;
    for (uint32_t i = t; i < n16; i += 256) {
        const qz_u128u v = *(const qz_u128u *)(src + head + 16u * i);
        qz_u128a w; w.v[0] = v.v[0]; w.v[1] = v.v[1]; w.v[2] = v.v[2]; w.v[3] = v.v[3];
        *(qz_u128a *)(dst + head + 16u * i) = w;
    }
    const uint32_t done = head + (n16 << 4);
    if (t < n - done) dst[done + t] = src[done + t];
}

/* block k (a workgroup each) from where the plan found it to dst + pos[k].offset; blocks that do not fit are left out */
QZ_KERNEL_MAX(256) qzk_blocks_pack_kernel(const uint8_t *streams, const uint8_t *plain, const qzk_blockpos *pos,
                                          const uint64_t *from, uint32_t nblocks, uint8_t *dst, uint64_t dst_cap)
{
    const uint32_t k = blockIdx.x;
    if (k >= nblocks) return;
    const qzk_blockpos b = pos[k];
    if (b.offset + b.size > dst_cap) return;
    qzk_block_copy16(dst + b.offset, (b.flags ? streams : plain) + from[k], b.size, threadIdx.x);
}

/* the stored blocks of a decompress call: job j copies len bytes from comp + in_off to out + out_off */
typedef struct { uint64_t in_off, out_off; uint32_t len, pad; } qzk_copyjob;
QZ_KERNEL_MAX(256) qzk_blocks_unpack_kernel(const uint8_t *comp, uint8_t *out, const qzk_copyjob *jobs, uint32_t njobs)
{
    const uint32_t j = blockIdx.x;
    if (j >= njobs) return;
    qzk_block_copy16(out + jobs[j].out_off, comp + jobs[j].in_off, jobs[j].len, threadIdx.x);
}

#endif
