/*
 * qz_frame_test.cpp — the host rules of the compress calls (qatzip_amd/csrc/qz_frame.h, qzd_slot_host.h) on the CPU: the
 * delivery rule, member framing, the folds of the crc out-parameter, the bounds, the slots of a round.  Every expected value
 * is written out here from the rule it checks.  Built and run by tests/test_qz_frame.py under the address and
 * undefined-behaviour sanitizers; no HIP, no library.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "qz_frame.h"

static int g_fail;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } } while (0)

static bool fit_is(QzFit f, uint32_t take, uint64_t bytes)
{
    if (f.take == take && f.bytes == bytes) return true;
    printf("  got take %u bytes %llu, want %u / %llu\n", f.take, (unsigned long long)f.bytes, take, (unsigned long long)bytes);
    return false;
}

/* ------------------------------------------------------------------ delivery */
static void test_delivery(void)
{
    static const uint32_t L[5] = {12, 0, 700, 7, 1};               /* 720 bytes; with 18 a piece 30, 18, 718, 25, 19 = 810 */
    /* no overhead */
    CHECK(fit_is(qz_fit(0, 0, 0, L, 5, 720), 5, 720));                 /* the total */
    CHECK(fit_is(qz_fit(0, 0, 0, L, 5, 719), 4, 719));                 /* one byte less: the last item stays behind */
    CHECK(fit_is(qz_fit(0, 0, 0, L, 5, 12), 2, 12));                   /* the first item - and the empty one behind it costs nothing */
    CHECK(fit_is(qz_fit(0, 0, 0, L, 5, 11), 0, 0));                    /* nothing fits */
    CHECK(fit_is(qz_fit(0, 0, 0, L, 5, 0), 0, 0));
    CHECK(fit_is(qz_fit(0, 0, 0, L, 5, 711), 2, 12));                  /* 712 would take the third */
    CHECK(fit_is(qz_fit(0, 0, 0, L, 5, 712), 3, 712));
    /* 18 bytes of framing an item */
    CHECK(fit_is(qz_fit(0, 18, 0, L, 5, 810), 5, 810));
    CHECK(fit_is(qz_fit(0, 18, 0, L, 5, 809), 4, 791));
    CHECK(fit_is(qz_fit(0, 18, 0, L, 5, 30), 1, 30));                  /* the first item; the empty one needs its 18 */
    CHECK(fit_is(qz_fit(0, 18, 0, L, 5, 29), 0, 0));
    CHECK(fit_is(qz_fit(0, 18, 0, L, 5, 0), 0, 0));
    CHECK(fit_is(qz_fit(0, 18, 0, L, 5, 47), 1, 30));                  /* the empty item at the boundary: 48 holds it, 47 does not */
    CHECK(fit_is(qz_fit(0, 18, 0, L, 5, 48), 2, 48));
    CHECK(fit_is(qz_fit(0, 0, 0, L, 0, 100), 0, 0));                   /* no items */
    /* one member: header 10, trailer 8 behind the last chunk */
    CHECK(fit_is(qz_fit(10, 0, 8, L, 5, 738), 5, 720));         /* 10 + 720 + 8 */
    CHECK(fit_is(qz_fit(10, 0, 8, L, 5, 737), 4, 719));         /* the chunks fit, the trailer does not: the last chunk goes back */
    CHECK(fit_is(qz_fit(10, 0, 8, L, 5, 730), 4, 719));
    CHECK(fit_is(qz_fit(10, 0, 8, L, 5, 729), 4, 719));         /* the last chunk does not fit anyway */
    CHECK(fit_is(qz_fit(10, 0, 8, L, 5, 728), 3, 712));         /* 10 + 712 + 7 is 729 */
    CHECK(fit_is(qz_fit(10, 0, 8, L, 5, 721), 2, 12));          /* 10 + 712 is 722 */
    CHECK(fit_is(qz_fit(10, 0, 0, L, 5, 730), 5, 720));         /* a call that leaves the member open has no trailer to fit */
    static const uint32_t one[1] = {700};
    CHECK(fit_is(qz_fit(10, 0, 8, one, 1, 718), 1, 700));
    CHECK(fit_is(qz_fit(10, 0, 8, one, 1, 717), 0, 0));         /* a single chunk without room for its trailer: nothing, no progress */
    CHECK(fit_is(qz_fit(10, 0, 8, one, 1, 710), 0, 0));
    /* what the call answers: 5 chunks of 16384, the last one 1000 bytes */
    const uint32_t hw = 16384, n = 4 * 16384 + 1000;
    QzDone d = qz_delivered(5, 5, n, hw); CHECK(d.rc == QZ_OK && d.used == 66536);
    d = qz_delivered(4, 5, n, hw); CHECK(d.rc == QZ_BUF_ERROR && d.used == 65536);
    d = qz_delivered(3, 5, n, hw); CHECK(d.rc == QZ_BUF_ERROR && d.used == 49152);
    d = qz_delivered(0, 5, n, hw); CHECK(d.rc == QZ_BUF_ERROR && d.used == 0);
    d = qz_delivered(1, 1, 1000, hw); CHECK(d.rc == QZ_OK && d.used == 1000);
    /* the give-back takes the item's framing with it: 810 + 8 fits, 810 alone gives the last item (19) back */
    CHECK(fit_is(qz_fit(0, 18, 8, L, 5, 818), 5, 810));
    CHECK(fit_is(qz_fit(0, 18, 8, L, 5, 817), 4, 791));
}

/* ------------------------------------------------------------------ framing */
static bool bytes_are(const unsigned char *got, const unsigned char *want, size_t n)
{
    if (!memcmp(got, want, n)) return true;
    printf("  got "); for (size_t i = 0; i < n; i++) printf("%02x ", got[i]);
    printf("\n want "); for (size_t i = 0; i < n; i++) printf("%02x ", want[i]);
    printf("\n");
    return false;
}

static void test_framing(void)
{
    static const unsigned lvls[4] = {1, 5, 6, 9};
    static const unsigned char xfl[4] = {4, 0, 0, 2};               /* zlib's gzip XFL: 4 fastest, 2 best */
    static const unsigned char zflg[4] = {0x01, 0x5e, 0x9c, 0xda};  /* 0x78 .. : FLEVEL 0 / 1 / 2 / 3 with its FCHECK */
    const uint32_t sum = 0xA1B2C3D4u, in_total = 0x00012345u, body = 0x00006789u;
    for (int i = 0; i < 4; i++) {
        unsigned char buf[64];
        /* GZIP, software path */
        unsigned char gz[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 3}; gz[8] = xfl[i];
        memset(buf, 0xee, sizeof(buf));
        CHECK(qz_member_open(buf, F_GZIP, (int)lvls[i], false) == 10);
        CHECK(bytes_are(buf, gz, 10) && buf[10] == 0xee);
        static const unsigned char gztr[8] = {0xD4, 0xC3, 0xB2, 0xA1, 0x45, 0x23, 0x01, 0x00};
        CHECK(qz_member_close(buf, buf + 10, F_GZIP, sum, in_total, body) == 8);
        CHECK(bytes_are(buf, gz, 10) && bytes_are(buf + 10, gztr, 8) && buf[18] == 0xee);      /* nothing to patch in a plain gzip header */
        /* GZIP_EXT, software path: sizes zero until the member is closed by the call that opened it */
        unsigned char gx[24] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 4, 255, 12, 0, 'Q', 'Z', 8, 0}; gx[8] = xfl[i];
        memset(buf, 0xee, sizeof(buf));
        CHECK(qz_member_open(buf, F_GZIP_EXT, (int)lvls[i], false) == 24);
        CHECK(bytes_are(buf, gx, 24) && buf[24] == 0xee);
        CHECK(qz_member_close(NULL, buf + 24, F_GZIP_EXT, sum, in_total, body) == 8);        /* closed by a later call: no patch */
        CHECK(bytes_are(buf, gx, 24) && bytes_are(buf + 24, gztr, 8) && buf[32] == 0xee);
        CHECK(qz_member_close(buf, buf + 24, F_GZIP_EXT, sum, in_total, body) == 8);
        static const unsigned char sizes[8] = {0x45, 0x23, 0x01, 0x00, 0x89, 0x67, 0x00, 0x00};
        CHECK(bytes_are(buf, gx, 16) && bytes_are(buf + 16, sizes, 8) && bytes_are(buf + 24, gztr, 8) && buf[32] == 0xee);
        /* ZLIB */
        const unsigned char zl[2] = {0x78, zflg[i]};
        memset(buf, 0xee, sizeof(buf));
        CHECK(qz_member_open(buf, F_ZLIB, (int)lvls[i], false) == 2);
        CHECK(bytes_are(buf, zl, 2) && buf[2] == 0xee && ((zl[0] << 8 | zl[1]) % 31) == 0);
        static const unsigned char ztr[4] = {0xA1, 0xB2, 0xC3, 0xD4};                          /* Adler-32, big-endian */
        CHECK(qz_member_close(buf, buf + 2, F_ZLIB, sum, in_total, body) == 4);
        CHECK(bytes_are(buf, zl, 2) && bytes_are(buf + 2, ztr, 4) && buf[6] == 0xee);
        /* 4B: the compressed length, once it is known */
        static const unsigned char z4[4] = {0, 0, 0, 0}, b4[4] = {0x89, 0x67, 0x00, 0x00};
        memset(buf, 0xee, sizeof(buf));
        CHECK(qz_member_open(buf, F_4B, (int)lvls[i], false) == 4);
        CHECK(bytes_are(buf, z4, 4) && buf[4] == 0xee);
        CHECK(qz_member_close(NULL, buf + 4, F_4B, sum, in_total, body) == 0);
        CHECK(bytes_are(buf, z4, 4) && buf[4] == 0xee);
        CHECK(qz_member_close(buf, buf + 4, F_4B, sum, in_total, body) == 0);
        CHECK(bytes_are(buf, b4, 4) && buf[4] == 0xee);
        /* RAW has no framing */
        memset(buf, 0xee, sizeof(buf));
        CHECK(qz_member_open(buf, F_RAW, (int)lvls[i], false) == 0 && qz_member_close(buf, buf, F_RAW, sum, in_total, body) == 0 && buf[0] == 0xee);
    }
    /* the hardware path: a complete member per chunk of cl bytes that deflated to zl; XFL 0, OS 255 whatever the level */
    const uint32_t cl = 0x00004000u, zl = 5, crc = 0x89ABCDEFu;
    static const unsigned char z[5] = {0xC1, 0xC2, 0xC3, 0xC4, 0xC5};
    unsigned char buf[64];
    static const unsigned char hg[23] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255, 0xC1, 0xC2, 0xC3, 0xC4, 0xC5,
                                         0xEF, 0xCD, 0xAB, 0x89, 0x00, 0x40, 0x00, 0x00};     /* CRC-32 and ISIZE of the chunk */
    static const unsigned char hx[37] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 255, 12, 0, 'Q', 'Z', 8, 0, 0x00, 0x40, 0, 0, 5, 0, 0, 0,
                                         0xC1, 0xC2, 0xC3, 0xC4, 0xC5, 0xEF, 0xCD, 0xAB, 0x89, 0x00, 0x40, 0x00, 0x00};
    static const unsigned char h4[9] = {5, 0, 0, 0, 0xC1, 0xC2, 0xC3, 0xC4, 0xC5};              /* the compressed length, no trailer */
    memset(buf, 0xee, sizeof(buf));
    CHECK(qz_member_open(buf, F_GZIP, 9, true) == 10 && bytes_are(buf, hg, 10) && buf[10] == 0xee);       /* XFL 0 whatever the level */
    CHECK(qz_member_open(buf, F_GZIP_EXT, -1, false) == 24 && buf[8] == 4 && buf[9] == 255);               /* below 2 is fastest, as an int */
    memset(buf, 0xee, sizeof(buf));
    CHECK(qz_hw_member(buf, F_GZIP, z, zl, cl, crc) == 23 && bytes_are(buf, hg, 23) && buf[23] == 0xee);
    memset(buf, 0xee, sizeof(buf));
    CHECK(qz_hw_member(buf, F_GZIP_EXT, z, zl, cl, crc) == 37 && bytes_are(buf, hx, 37) && buf[37] == 0xee);
    memset(buf, 0xee, sizeof(buf));
    CHECK(qz_hw_member(buf, F_4B, z, zl, cl, crc) == 9 && bytes_are(buf, h4, 9) && buf[9] == 0xee);
}

/* ------------------------------------------------------------------ the crc out-parameter */
/* zlib's crc32_combine, bit by bit: crc1's register goes through 8 * len2 zero bits of the reflected CRC-32, crc2 is added */
static uint32_t combine_bits(uint32_t crc1, uint32_t crc2, uint64_t len2)
{
    for (uint64_t i = 0; i < 8 * len2; i++) crc1 = (crc1 >> 1) ^ ((crc1 & 1) ? 0xEDB88320u : 0);
    return crc1 ^ crc2;
}

/* the combines the header links against (the library's are in the device layer): the one above, and zlib's adler32_combine */
extern "C" uint32_t qzd_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) { return combine_bits(crc1, crc2, len2); }
extern "C" uint32_t qzd_adler32_combine(uint32_t ad1, uint32_t ad2, uint64_t len2)
{
    const uint32_t B = 65521, rem = (uint32_t)(len2 % B);
    uint32_t s1 = (ad1 & 0xffff) + (ad2 & 0xffff) + B - 1, s2 = (rem * (ad1 & 0xffff)) % B + (ad1 >> 16) + (ad2 >> 16) + B - rem;
    if (s1 >= B) s1 -= B;
    if (s1 >= B) s1 -= B;
    if (s2 >= 2 * B) s2 -= 2 * B;
    if (s2 >= B) s2 -= B;
    return s1 | s2 << 16;
}

/* three chunks of 4096, 4096 and 1000 bytes: a call of 9192 bytes at hw 4096 */
static unsigned long fold_all(int fmt, unsigned long start, const uint32_t *c, uint32_t *run_out = NULL)
{
    unsigned long crc = start;
    const uint32_t run = qz_fold_chunks(&crc, fmt, fmt == F_ZLIB ? 1u : 0u, c, c, 3, 9192, 4096);
    if (run_out) *run_out = run;
    return crc;
}

static void test_fold(void)
{
    /* the combine itself on a known pair: crc32("123456789") = cbf43926, crc32("12345") = cbf53a1c, crc32("6789") = 9dbabf87 */
    CHECK(combine_bits(0xcbf53a1cu, 0x9dbabf87u, 4) == 0xcbf43926u);
    static const uint32_t c[3] = {0x11111111u, 0x2468ACE0u, 0xDEADBEEFu};
    const uint32_t X = 0x0BADF00Du;
    /* RAW: the chunks' CRCs one after the other, whatever *crc was */
    uint32_t run = 77;
    CHECK(fold_all(F_RAW, 0, c, &run) == combine_bits(combine_bits(combine_bits(0, c[0], 4096), c[1], 4096), c[2], 1000) && run == 0);
    CHECK(fold_all(F_RAW, X, c) == combine_bits(combine_bits(combine_bits(X, c[0], 4096), c[1], 4096), c[2], 1000));
    /* GZIP: the stream's running sum after each chunk, folded as if it covered all of the call so far */
    const uint32_t s0 = combine_bits(0, c[0], 4096), s1 = combine_bits(s0, c[1], 4096), s2 = combine_bits(s1, c[2], 1000);
    CHECK(fold_all(F_GZIP, 0, c, &run) == combine_bits(combine_bits(s0, s1, 8192), s2, 9192) && run == s2);     /* 0 takes s0 */
    CHECK(fold_all(F_GZIP, X, c) == combine_bits(combine_bits(combine_bits(X, s0, 4096), s1, 8192), s2, 9192));
    CHECK(fold_all(F_GZIP_EXT, X, c) == fold_all(F_GZIP, X, c));
    /* the first two chunks alone, and no crc asked for: the running sum all the same */
    CHECK(qz_fold_chunks(NULL, F_GZIP, 0, c, NULL, 2, 9192, 4096) == s1);
    /* ZLIB: the running sum is an Adler-32 from 1 - adler32("a") 00620062, ("bc") 012900c6, ("abc") 024d0127 */
    CHECK(qzd_adler32_combine(0x00620062u, 0x012900c6u, 2) == 0x024d0127u);
    const uint32_t a0 = qzd_adler32_combine(1, c[0], 4096), a1 = qzd_adler32_combine(a0, c[1], 4096), a2 = qzd_adler32_combine(a1, c[2], 1000);
    CHECK(fold_all(F_ZLIB, X, c, &run) == combine_bits(combine_bits(combine_bits(X, a0, 4096), a1, 8192), a2, 9192) && run == a2);
    /* 4B keeps no sum: 1 takes its place */
    CHECK(fold_all(F_4B, 0, c, &run) == combine_bits(combine_bits(1, 1, 8192), 1, 9192) && run == 0);
    CHECK(fold_all(F_4B, X, c) == combine_bits(combine_bits(combine_bits(X, 1, 4096), 1, 8192), 1, 9192));
    /* the hardware path: only the call's first chunk may take */
    unsigned long crc = 0;
    qz_crc_fold_hw(&crc, 0, c[0], 4096); CHECK(crc == c[0]);
    crc = 0;
    qz_crc_fold_hw(&crc, 1, c[1], 4096); CHECK(crc == combine_bits(0, c[1], 4096));
    crc = X;
    qz_crc_fold_hw(&crc, 0, c[0], 4096); CHECK(crc == combine_bits(X, c[0], 4096));
    /* LZ4s: always combined */
    crc = 0;
    qz_crc_fold_lz4s(&crc, c[2], 1000); CHECK(crc == combine_bits(0, c[2], 1000));
    crc = X;
    qz_crc_fold_lz4s(&crc, c[2], 1000); CHECK(crc == combine_bits(X, c[2], 1000));
}

/* ------------------------------------------------------------------ bounds and rounds */
static uint64_t parent_deflate_bound(uint64_t in, uint64_t nchunks, uint32_t hw) { return in + nchunks * (5ull * (hw / 32767 + 2) + 16) + 64; }
static uint64_t parent_linked_bound(uint64_t n) { const uint64_t blocks = (n + 65535) >> 16; return 19 + 4 * blocks + n + 8; }

static void test_bounds(void)
{
    CHECK(qz_deflate_bound(0, 1, 65536) == 100 && parent_deflate_bound(0, 1, 65536) == 100);                  /* 5 * (2 + 2) + 16 + 64 */
    CHECK(qz_deflate_bound(70000, 2, 65536) == 70136 && parent_deflate_bound(70000, 2, 65536) == 70136);       /* + 2 * 36 + 64 */
    CHECK(qz_deflate_bound(1u << 20, 64, 16384) == 1050304 && parent_deflate_bound(1u << 20, 64, 16384) == 1050304);   /* + 64 * 26 + 64 */
    CHECK(qzd_lz4_linked_bound(65537) == 65572 && parent_linked_bound(65537) == 65572);                       /* 19 + 2 * 4 + n + 8 */
    CHECK(qzd_lz4_linked_bound(0x7fff0000ull) == 2147549207ull && parent_linked_bound(0x7fff0000ull) == 2147549207ull);   /* 32767 blocks */
}

static void test_batch(void)
{
    const uint64_t G = 1ull << 30;
    CHECK(QZD_SLOT_GIGABYTE == G && QZD_SLOT_ROUND == 16384);
    /* one item is one slot, however large */
    CHECK(qzd_slot_batch(1, 1056, 0) == 1 && qzd_slot_batch(1, 1056, G) == 1);
    CHECK(qzd_slot_batch(1, 65632, 0) == 1 && qzd_slot_batch(1, (1u << 30) + 112, G) == 1);
    /* LZ4 frames of 64 KB: stride 65536 + 15 + 4 + 8 + 64 to 16 bytes = 65632.  lz4_compress_frames_impl passes no budget
     * up to 64 KB frames, so a round keeps 16384 slots (1 075 314 688 bytes); the gigabyte would make it 16360 */
    CHECK(qzd_slot_batch(20000, 65632, 0) == 16384);
    CHECK(qzd_slot_batch(20000, 65632, G) == 16360);
    /* ... and the gigabyte for linked frames (hardware framing above 64 KB): 1 MB frames, stride 1048576 + 15 + 64 + 8 + 64 to 16 */
    CHECK(qzd_slot_batch(5000, 1048736, G) == 1023);
    /* qzd_lz4s_compress_blocks: the gigabyte.  512 KB blocks: 4 + 524288 + 2056 + 36 + 16 = 526400, a multiple of 16 */
    CHECK(qzd_slot_batch(5000, 526400, G) == (uint32_t)(G / 526400) && G / 526400 == 2039);
    /* 1 KB blocks: 4 + 1024 + 4 + 4 + 16 = 1052 -> 1056: all 16384 fit */
    CHECK(qzd_slot_batch(16384, 1056, G) == 16384);
    CHECK(qzd_slot_batch(16385, 1056, G) == 16384);
    /* qzd_zstd_compress_frames and qzd_zstd_encode_frames: the gigabyte.  128 KB frames: 131072 + 12 + 64 to 16 = 131152 */
    CHECK(qzd_slot_batch(20000, 131152, G) == 8187);
    CHECK(qzd_slot_batch(100, 131152, G) == 100);
    /* which budget lz4_compress_frames_impl passes: none for one-block frames, the gigabyte from the first linked size on */
    CHECK(qzd_lz4_slot_budget(1024) == 0 && qzd_lz4_slot_budget(65536) == 0);
    CHECK(qzd_lz4_slot_budget(65537) == G && qzd_lz4_slot_budget(1u << 20) == G && qzd_lz4_slot_budget(1u << 30) == G);
    CHECK(qzd_slot_batch(20000, 65632, qzd_lz4_slot_budget(65536)) == 16384);
    CHECK(qzd_slot_batch(5000, 1048736, qzd_lz4_slot_budget(1u << 20)) == 1023);
    /* (lz4hc_impl does not come here: rounds of QZD_HC_BATCH = 4096 blocks) */
}

int main(void)
{
    test_delivery();
    test_framing();
    test_fold();
    test_bounds();
    test_batch();
    if (g_fail) { printf("qz_frame_test: %d FAILED\n", g_fail); return 1; }
    printf("qz_frame_test: ok\n");
    return 0;
}
