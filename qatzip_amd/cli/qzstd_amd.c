/*
 * qzstd-amd — the compress path of the reference's utils/qzstd: a file in, <file>.zst out, one zstd frame per hw_buff_sz
 * chunk, written by a zstd session (include/qzamd_zstd.h) on the GPU.  Plain C against the two headers, linked like any
 * application.  The file is read in pieces of whole chunks and the frames are concatenated, so the output is what one call
 * over the whole file would give.
 * --decompress <file.zst> is the other direction, on a zstd decode session (include/qzamd_zstd_dec.h): the file is read in
 * pieces that end on frame boundaries (qzd_zstdd_host.h walks the block headers) and decoded on the GPU, frames of any zstd
 * writer.  The short -d keeps its old answer (exit 2, "use zstd -d"): scripts and tests rely on it.
 */
#include <errno.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "qatzip.h"
#include "qzamd_zstd.h"
#include "qzamd_zstd_dec.h"
#include "qzamd_zstd_seq.h"
#include "qzamd_zstd_parse.h"
#include "../csrc/qzd_zstdd_host.h"

#define PIECE_BYTES (64u * 1024 * 1024)
#define OUT_PIECE_BYTES (256u * 1024 * 1024)    /* frames are handed to qzDecompress until their output passes this */

static void usage(FILE *f)
{
    fprintf(f, "usage: qzstd-amd [options] <file>\n"
               "  compresses <file> to <file>.zst, one zstd frame per chunk, and removes <file>\n"
               "  -C <bytes>   hw_buff_sz, the chunk: a power of two in 1024 .. 131072 (default 65536)\n"
               "  -L <level>   comp_lvl 1-12 (default 1; every level runs the same parse)\n"
               "  -m <3|4>     lz4s_mini_match (default 3)\n"
               "  -o <name>    write to <name> instead of <file>.zst\n"
               "  -k           keep <file>\n"
               "  --seq-tables the sequence tables of a frame Predefined, RLE or FSE_Compressed, whichever is smallest\n"
               "  --repeat-offsets\n"
               "               offsets coded against the repeat-offset history\n"
               "  --parse-depth <N>\n"
               "               0 (default) the parse of LZ4s sessions; 1 .. 256 a hash-chain lazy parse with N search attempts\n"
               "               per position, offsets back to the chunk's start and repeat offsets weighed in\n"
               "  -d           not offered under this spelling (exit 2): use --decompress, or zstd -d\n"
               "  --decompress <file.zst>\n"
               "               decode <file.zst> (zstd and skippable frames of any writer, no dictionaries) to <file>,\n"
               "               or to the name given with -o, and remove <file.zst> unless -k; -C, -L, -m are ignored\n"
               "  -h           this text\n");
}

/* --decompress: returns the exit status */
static int decompress_file(QzSession_T *sess, const char *iname, const char *oname)
{
    int status = 1, created = 0;
    FILE *in = fopen(iname, "rb"), *out = NULL;
    size_t cap = PIECE_BYTES, have = 0, dcap = 0;
    unsigned char *src = (unsigned char *)malloc(cap), *dst = NULL;
    int eof = 0;
    if (!in) { fprintf(stderr, "qzstd-amd: %s: %s\n", iname, strerror(errno)); goto done; }
    out = fopen(oname, "wb");
    if (!out) { fprintf(stderr, "qzstd-amd: %s: %s\n", oname, strerror(errno)); goto done; }
    created = 1;
    if (!src) { fprintf(stderr, "qzstd-amd: out of memory\n"); goto done; }
    for (;;) {
        if (!eof && have < cap) {
            const size_t got = fread(src + have, 1, cap - have, in);
            if (ferror(in)) { fprintf(stderr, "qzstd-amd: %s: read error\n", iname); goto done; }
            have += got;
            if (got == 0) eof = 1;
        }
        if (have == 0 && eof) break;
        /* the whole frames at the front of the buffer, as many as keep the output of one hand-over under OUT_PIECE_BYTES */
        size_t in_sum = 0; uint64_t out_sum = 0;
        while (in_sum < have) {
            uint64_t content = 0, bound = 0; bool hc = false;
            const int64_t ext = qzd_zd_frame_extent(src + in_sum, have - in_sum, &content, &hc, &bound);
            if (ext == QZD_ZD_MALFORMED) { fprintf(stderr, "qzstd-amd: %s: not a zstd frame at its byte %zu of this piece\n", iname, in_sum); goto done; }
            if (ext < 0) break;
            const uint64_t need = hc ? content : bound;
            if (need > 0xffff0000ull) { fprintf(stderr, "qzstd-amd: %s: a frame of %llu bytes is more than one call takes\n", iname, (unsigned long long)need); goto done; }
            if (in_sum && out_sum + need > OUT_PIECE_BYTES) break;
            in_sum += (size_t)ext; out_sum += need;
        }
        if (in_sum == 0) {                                          /* the first frame is not whole yet */
            if (eof) { fprintf(stderr, "qzstd-amd: %s: the last frame is cut\n", iname); goto done; }
            if (have == cap) {
                if (cap >= 0xc0000000ull) { fprintf(stderr, "qzstd-amd: %s: a frame is more than one call takes\n", iname); goto done; }
                unsigned char *g = (unsigned char *)realloc(src, cap * 2);
                if (!g) { fprintf(stderr, "qzstd-amd: out of memory\n"); goto done; }
                src = g; cap *= 2;
            }
            continue;
        }
        if (out_sum + 1 > dcap) {
            free(dst);
            dcap = (size_t)out_sum + 1;
            dst = (unsigned char *)malloc(dcap);
            if (!dst) { fprintf(stderr, "qzstd-amd: out of memory\n"); goto done; }
        }
        size_t used = 0;
        while (used < in_sum) {                                     /* (a frame without a content size comes back alone) */
            unsigned sl = (unsigned)(in_sum - used), dl = (unsigned)(dcap > 0xffffffffu ? 0xffffffffu : dcap);
            const int rc = qzDecompress(sess, src + used, &sl, dst, &dl);
            if (rc != QZ_OK || sl == 0) { fprintf(stderr, "qzstd-amd: %s: qzDecompress failed (%d)\n", iname, rc); goto done; }
            if (fwrite(dst, 1, dl, out) != dl) { fprintf(stderr, "qzstd-amd: %s: write error\n", oname); goto done; }
            used += sl;
        }
        memmove(src, src + in_sum, have - in_sum);
        have -= in_sum;
    }
    if (fclose(out) != 0) { out = NULL; fprintf(stderr, "qzstd-amd: %s: write error\n", oname); goto done; }
    out = NULL;
    status = 0;
done:
    if (in) fclose(in);
    if (out) fclose(out);
    free(src); free(dst);
    if (status != 0 && created) unlink(oname);
    return status;
}

int main(int argc, char **argv)
{
    unsigned hw = 65536, level = 1, mm = 3;
    const char *oname = NULL;
    int keep = 0, c, decompress = 0;
    unsigned seq_flags = 0, parse_depth = 0;
    static const struct option longopts[] = { { "decompress", no_argument, NULL, 'D' }, { "seq-tables", no_argument, NULL, 'T' },
                                              { "repeat-offsets", no_argument, NULL, 'R' }, { "parse-depth", required_argument, NULL, 'P' },
                                              { NULL, 0, NULL, 0 } };
    while ((c = getopt_long(argc, argv, "C:L:m:o:kdh", longopts, NULL)) != -1) {
        switch (c) {
        case 'D': decompress = 1; break;
        case 'T': seq_flags |= QZ_ZSTD_SEQ_FSE_TABLES; break;
        case 'R': seq_flags |= QZ_ZSTD_SEQ_REPEAT_OFFSETS; break;
        case 'P': {
            char *end = NULL;
            const unsigned long v = strtoul(optarg, &end, 0);
            if (!*optarg || *end || v > QZ_ZSTD_PARSE_DEPTH_MAX) { fprintf(stderr, "qzstd-amd: --parse-depth takes 0 .. %u\n", QZ_ZSTD_PARSE_DEPTH_MAX); return 2; }
            parse_depth = (unsigned)v;
            break;
        }
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
    if (decompress) {
        const size_t il = strlen(iname);
        if (!oname) {
            if (il < 5 || strcmp(iname + il - 4, ".zst")) { fprintf(stderr, "qzstd-amd: %s has no .zst suffix: name the output with -o\n", iname); return 2; }
            auto_name = (char *)malloc(il);
            if (!auto_name) return 1;
            memcpy(auto_name, iname, il - 4); auto_name[il - 4] = 0;
            oname = auto_name;
        }
        QzSession_T dsess;
        QzSessionParamsLZ4S_T dp;
        memset(&dsess, 0, sizeof(dsess));
        int drc = qzInit(&dsess, 0);
        if (drc != QZ_OK && drc != QZ_DUPLICATE) { fprintf(stderr, "qzstd-amd: qzInit failed (%d)\n", drc); return 1; }
        qzGetDefaultsLZ4S(&dp);
        dp.common_params.comp_algorithm = QZ_LZ4s;
        dp.common_params.direction = QZ_DIR_DECOMPRESS;
        dp.common_params.hw_buff_sz = 65536;
        dp.qzCallback = NULL; dp.qzCallback_external = NULL;
        drc = qzSetupSessionZstdDecAMD(&dsess, &dp);
        if (drc != QZ_OK) { fprintf(stderr, "qzstd-amd: no decode session (%d)\n", drc); return 1; }
        const int st = decompress_file(&dsess, iname, oname);
        qzTeardownSession(&dsess);
        qzClose(&dsess);
        if (st == 0 && !keep) unlink(iname);
        free(auto_name);
        return st;
    }
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
    if (seq_flags && qzSetSessionZstdSeqAMD(&sess, seq_flags) != QZ_OK) { fprintf(stderr, "qzstd-amd: the sequence options are refused\n"); qzTeardownSession(&sess); return 2; }
    if (parse_depth && qzSetSessionZstdParseAMD(&sess, parse_depth) != QZ_OK) { fprintf(stderr, "qzstd-amd: the parse depth is refused\n"); qzTeardownSession(&sess); return 2; }

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
