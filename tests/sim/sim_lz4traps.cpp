/*
 * sim_lz4traps.cpp - a program of its own for the sanitizers: reads trap inputs (u32le length + bytes, one after the other)
 * from the file named on its command line, puts each one into a heap buffer of EXACTLY its length and runs the three LZ4
 * level-1 compressors on it through the SIMT emulator: qzk_lz4c_kernel, qzk_lz4c_pull_kernel (one frame per call) and,
 * above 64 KB, qzk_lz4c_linked_kernel.  Built with -fsanitize=address,undefined a read past an input's end stops it: that
 * is what this program is for.  Its only check of the bytes is that the two independent-block kernels write the same frame
 * (and that a linked frame's length is plausible); the comparison with liblz4's pinned bytes is
 * tests/test_sim_lz4_traps.py's.  TEST INFRASTRUCTURE.
 */
#include "sim_driver.cpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned count = 0, failures = 0;
    uint8_t lenb[4];
    while (fread(lenb, 1, 4, f) == 4) {
        const uint32_t n = lenb[0] | lenb[1] << 8 | lenb[2] << 16 | (uint32_t)lenb[3] << 24;
        uint8_t *src = (uint8_t *)malloc(n ? n : 1);
        if (n && fread(src, 1, n, f) != n) return 2;
        if (n <= 65536) {
            const uint32_t fs = n ? n : 65536, stride = (fs + 15 + 4 + 8 + 64 + 15) & ~15u;
            uint8_t *a = (uint8_t *)calloc(stride, 1), *b = (uint8_t *)calloc(stride, 1);
            uint32_t la = 0, lb = 0;
            sim_lz4c(src, n, fs, a, stride, &la);
            sim_lz4c_pull(src, n, fs, b, stride, &lb, 1);
            if (la != lb || la > stride || memcmp(a, b, la)) { failures++; printf("input %u (n = %u): the two kernels differ\n", count, n); }
            free(a); free(b);
        } else {
            uint8_t *o = (uint8_t *)calloc((size_t)n + n / 255 + 4096, 1);
            uint32_t lo = 0;
            sim_lz4c_linked(src, n, o, &lo);
            if (lo < 23 || lo > n + n / 255 + 4096) { failures++; printf("input %u (n = %u): length %u\n", count, n, lo); }
            free(o);
        }
        free(src);
        count++;
    }
    fclose(f);
    printf("%u inputs, %u failures\n", count, failures);
    return failures ? 1 : 0;
}
