/*
 * qzstd-amd — the compress path of the reference's utils/qzstd: a file in, <file>.zst out, one zstd frame per hw_buff_sz
 * chunk, written by a zstd session (include/qzamd_zstd.h) on the GPU.  Plain C against the two headers, linked like any
 * application.  The file is read in pieces of whole chunks and the frames are concatenated, so the output is what one call
 * over the whole file would give.  There is no decoder here: any zstd reads the result (zstd -d).
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "qatzip.h"
#include "qzamd_zstd.h"

#define PIECE_BYTES (64u * 1024 * 1024)

static void usage(FILE *f)
{
    fprintf(f, "usage: qzstd-amd [options] <file>\n"
               "  compresses <file> to <file>.zst, one zstd frame per chunk, and removes <file>\n"
               "  -C <bytes>   hw_buff_sz, the chunk: a power of two in 1024 .. 131072 (default 65536)\n"
               "  -L <level>   comp_lvl 1-12 (default 1; every level runs the same parse)\n"
               "  -m <3|4>     lz4s_mini_match (default 3)\n"
               "  -o <name>    write to <name> instead of <file>.zst\n"
               "  -k           keep <file>\n"
               "  -d           not offered: decompress with zstd -d\n"
               "  -h           this text\n");
}

int main(int argc, char **argv)
{
    unsigned hw = 65536, level = 1, mm = 3;
    const char *oname = NULL;
    int keep = 0, c;
    while ((c = getopt(argc, argv, "C:L:m:o:kdh")) != -1) {
        switch (c) {
        case 'C': hw = (unsigned)strtoul(optarg, NULL, 0); break;
        case 'L': level = (unsigned)strtoul(optarg, NULL, 0); break;
        case 'm': mm = (unsigned)strtoul(optarg, NULL, 0); break;
        case 'o': oname = optarg; break;
        case 'k': keep = 1; break;
        case 'd': fprintf(stderr, "qzstd-amd: decompression is not offered here; use zstd -d\n"); return 2;
        case 'h': usage(stdout); return 0;
        default: usage(stderr); return 2;
        }
    }
    if (optind + 1 != argc) { usage(stderr); return 2; }
    const char *iname = argv[optind];
    char *auto_name = NULL;
    if (!oname) {
        auto_name = (char *)malloc(strlen(iname) + 5);
        if (!auto_name) return 1;
        sprintf(auto_name, "%s.zst", iname);
        oname = auto_name;
    }

    QzSession_T sess;
    QzSessionParamsLZ4S_T p;
    memset(&sess, 0, sizeof(sess));
    int rc = qzInit(&sess, 0);
    if (rc != QZ_OK && rc != QZ_DUPLICATE) { fprintf(stderr, "qzstd-amd: qzInit failed (%d)\n", rc); return 1; }
    qzGetDefaultsLZ4S(&p);
    p.common_params.comp_algorithm = QZ_LZ4s;
    p.common_params.direction = QZ_DIR_COMPRESS;
    p.common_params.hw_buff_sz = hw;
    p.common_params.comp_lvl = level;
    p.lz4s_mini_match = mm;
    p.qzCallback = NULL; p.qzCallback_external = NULL;
    rc = qzSetupSessionZstdAMD(&sess, &p);
    if (rc != QZ_OK) { fprintf(stderr, "qzstd-amd: these parameters are refused (%d): -C a power of two in 1024 .. 131072, -L 1-12, -m 3 or 4\n", rc); return 2; }

    int status = 1, created = 0;
    FILE *in = fopen(iname, "rb"), *out = NULL;
    unsigned char *src = NULL, *dst = NULL;
    const unsigned piece = PIECE_BYTES / hw * hw;               /* whole chunks */
    const unsigned cap = qzMaxCompressedLength(piece, &sess);
    if (!in) { fprintf(stderr, "qzstd-amd: %s: %s\n", iname, strerror(errno)); goto done; }
    out = fopen(oname, "wb");
    if (!out) { fprintf(stderr, "qzstd-amd: %s: %s\n", oname, strerror(errno)); goto done; }
    created = 1;
    src = (unsigned char *)malloc(piece);
    dst = (unsigned char *)malloc(cap);
    if (!src || !dst || !cap) { fprintf(stderr, "qzstd-amd: out of memory\n"); goto done; }
    for (;;) {
        const size_t got = fread(src, 1, piece, in);
        if (ferror(in)) { fprintf(stderr, "qzstd-amd: %s: read error\n", iname); goto done; }
        if (got == 0) break;
        unsigned sl = (unsigned)got, dl = cap;
        rc = qzCompress(&sess, src, &sl, dst, &dl, 1);
        if (rc != QZ_OK || sl != got) { fprintf(stderr, "qzstd-amd: qzCompress failed (%d)\n", rc); goto done; }
        if (fwrite(dst, 1, dl, out) != dl) { fprintf(stderr, "qzstd-amd: %s: write error\n", oname); goto done; }
        if (got < piece) break;
    }
    if (fclose(out) != 0) { out = NULL; fprintf(stderr, "qzstd-amd: %s: write error\n", oname); goto done; }
    out = NULL;
    status = 0;
done:
    if (in) fclose(in);
    if (out) fclose(out);
    free(src); free(dst);
    qzTeardownSession(&sess);
    qzClose(&sess);
    if (status == 0 && !keep) unlink(iname);
    if (status != 0 && created) unlink(oname);                  /* no half-written output is left behind */
    free(auto_name);
    return status;
}
