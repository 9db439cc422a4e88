/*
 * qz_unframe_test.cpp — the host rules of the decompress calls (qatzip_amd/csrc/qz_unframe.h) on the CPU: the member header,
 * sized gzip-ext members, one member as one inflate segment, the LZ4 frame extent, the frame plan and its result check, the
 * folds of the crc out-parameter.  Every expected value is written out here from the rule it checks; every input lies in an
 * allocation that ends where the input ends, so a read past it stops the run.  Built and run by tests/test_qz_unframe.py
 * under the address and undefined-behaviour sanitizers; no HIP, no library.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "qz_unframe.h"

static int g_fail;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } } while (0)

typedef std::vector<unsigned char> Bytes;
static Bytes operator+(Bytes a, const Bytes &b) { a.insert(a.end(), b.begin(), b.end()); return a; }
static Bytes le32(uint32_t v) { return Bytes{(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)}; }
static Bytes fill(size_t n, unsigned char v) { return Bytes(n, v); }

/* the first n bytes of b (all of it by default) at the END of an allocation of their own: p[n] is out of bounds */
struct Exact {
    unsigned char *base, *p; uint32_t n;
    Exact(const Bytes &b, size_t len = (size_t)-1)
    {
        n = (uint32_t)(len == (size_t)-1 ? b.size() : len);
        base = (unsigned char *)malloc(n ? n : 1);
        p = base + (n ? 0 : 1);
        if (n) memcpy(p, b.data(), n);
    }
    ~Exact() { free(base); }
    Exact(const Exact &) = delete;
};

/* ------------------------------------------------------------------ the member header */
static int hdr(int fmt, const Bytes &b, uint32_t *es, uint32_t *ed, size_t len = (size_t)-1)
{
    Exact e(b, len);
    *es = *ed = 0xdeadbeefu;                                        /* both are always written */
    return parse_header(fmt, e.p, e.n, es, ed);
}
static bool hdr_is(int fmt, const Bytes &b, int want, uint32_t want_es = 0, uint32_t want_ed = 0, size_t len = (size_t)-1)
{
    uint32_t es, ed;
    const int got = hdr(fmt, b, &es, &ed, len);
    if (got == want && es == want_es && ed == want_ed) return true;
    printf("  got %d (%u, %u), want %d (%u, %u)\n", got, es, ed, want, want_es, want_ed);
    return false;
}
/* gzip's ten bytes with FLG flg, and gzip-ext's 24: FEXTRA, XLEN 12, 'Q' 'Z', 8, the uncompressed and the compressed size */
static Bytes gz10(unsigned char flg) { return Bytes{0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 255}; }
static Bytes gzext(uint32_t usz, uint32_t csz) { return gz10(4) + Bytes{12, 0, 'Q', 'Z', 8, 0} + le32(usz) + le32(csz); }

static void test_header(void)
{
    /* each format's minimal header */
    CHECK(hdr_is(F_RAW, Bytes{}, 0));
    CHECK(hdr_is(F_4B, Bytes{9, 9, 9, 9}, 4) && hdr_is(F_4B, Bytes{9, 9, 9}, QZ_DATA_ERROR) && hdr_is(F_4B, Bytes{}, QZ_DATA_ERROR));
    CHECK(hdr_is(F_ZLIB, Bytes{0x78, 0x9c}, 2) && hdr_is(F_ZLIB, Bytes{0x78, 0x01}, 2));       /* 0x789c = 31 * 996, 0x7801 = 31 * 991 */
    CHECK(hdr_is(F_ZLIB, Bytes{0x78}, QZ_DATA_ERROR) && hdr_is(F_ZLIB, Bytes{}, QZ_DATA_ERROR));
    CHECK(hdr_is(F_ZLIB, Bytes{0x78, 0x9d}, QZ_DATA_ERROR));                                   /* bad FCHECK */
    CHECK((0x7820 % 31) == 0 && hdr_is(F_ZLIB, Bytes{0x78, 0x20}, QZ_DATA_ERROR));             /* FCHECK good, FDICT set */
    CHECK((0x7918 % 31) == 0 && hdr_is(F_ZLIB, Bytes{0x79, 0x18}, QZ_DATA_ERROR));             /* FCHECK good, CM 9 */
    CHECK(hdr_is(F_GZIP, gz10(0), 10) && hdr_is(F_GZIP_EXT, gz10(0), 10));                     /* the two gzip formats read the same headers */
    CHECK(hdr_is(F_GZIP, gz10(0) + fill(5, 0xaa), 10));
    CHECK(hdr_is(F_GZIP, gz10(0), QZ_DATA_ERROR, 0, 0, 9));
    CHECK(hdr_is(F_GZIP_EXT, gzext(0x00010000u, 0x1234u), 24, 0x00010000u, 0x1234u));
    CHECK(hdr_is(F_GZIP, gzext(7, 3) + fill(3, 0), 24, 7, 3));
    Bytes bad = gz10(0); bad[0] = 0x1e; CHECK(hdr_is(F_GZIP, bad, QZ_DATA_ERROR));
    bad = gz10(0); bad[1] = 0x8c; CHECK(hdr_is(F_GZIP, bad, QZ_DATA_ERROR));
    bad = gz10(0); bad[2] = 7; CHECK(hdr_is(F_GZIP, bad, QZ_DATA_ERROR));                      /* CM is not deflate */
    CHECK(hdr_is(F_GZIP, gz10(0x20), QZ_DATA_ERROR) && hdr_is(F_GZIP, gz10(0x40), QZ_DATA_ERROR) && hdr_is(F_GZIP, gz10(0x80), QZ_DATA_ERROR));
    CHECK(hdr_is(F_GZIP, gz10(0x01), 10));                                                     /* FTEXT means nothing here */
    /* FEXTRA that is not 'QZ', or not 8 bytes of it: skipped, no sizes */
    CHECK(hdr_is(F_GZIP_EXT, gz10(4) + Bytes{12, 0, 'A', 'B', 8, 0} + le32(7) + le32(3), 24));
    CHECK(hdr_is(F_GZIP_EXT, gz10(4) + Bytes{12, 0, 'Q', 'Z', 9, 0} + le32(7) + le32(3), 24));
    CHECK(hdr_is(F_GZIP_EXT, gz10(4) + Bytes{0, 0}, 12));
    CHECK(hdr_is(F_GZIP_EXT, gz10(4) + Bytes{3, 0, 'Q', 'Z', 8}, 15));                         /* xl 3: 'Q' 'Z' are there, the sizes are not read */
    /* 'QZ' with xl != 12 */
    CHECK(hdr_is(F_GZIP_EXT, gz10(4) + Bytes{14, 0, 'Q', 'Z', 8, 0} + le32(7) + le32(3) + Bytes{0, 0}, 26));
    CHECK(hdr_is(F_GZIP_EXT, gz10(4) + Bytes{11, 0, 'Q', 'Z', 8, 0} + le32(7) + Bytes{3, 0, 0}, 23));
    /* XLEN cut, and an extra field that runs past the end */
    CHECK(hdr_is(F_GZIP_EXT, gz10(4) + Bytes{12}, QZ_DATA_ERROR) && hdr_is(F_GZIP_EXT, gz10(4) + Bytes{0xff, 0xff} + fill(20, 1), QZ_DATA_ERROR));
    /* FNAME and FCOMMENT: terminated, and unterminated at the buffer's end */
    CHECK(hdr_is(F_GZIP, gz10(8) + Bytes{'a', 'b', 0}, 13) && hdr_is(F_GZIP, gz10(8) + Bytes{'a', 'b'}, QZ_DATA_ERROR));
    CHECK(hdr_is(F_GZIP, gz10(16) + Bytes{'c', 0}, 12) && hdr_is(F_GZIP, gz10(16) + Bytes{'c'}, QZ_DATA_ERROR));
    CHECK(hdr_is(F_GZIP, gz10(8) + Bytes{0}, 11) && hdr_is(F_GZIP, gz10(8), QZ_DATA_ERROR));
    CHECK(hdr_is(F_GZIP, gz10(24) + Bytes{'a', 0, 'c', 'd', 0, 0x55}, 15));
    CHECK(hdr_is(F_GZIP, gz10(24) + Bytes{'a', 0, 'c', 'd'}, QZ_DATA_ERROR) && hdr_is(F_GZIP, gz10(24) + Bytes{'a', 0}, QZ_DATA_ERROR));
    /* FHCRC: two bytes, there or running past the end */
    CHECK(hdr_is(F_GZIP, gz10(2) + Bytes{1, 2}, 12) && hdr_is(F_GZIP, gz10(2) + Bytes{1}, QZ_DATA_ERROR) && hdr_is(F_GZIP, gz10(2), QZ_DATA_ERROR));
    /* everything at once: 10 + (2 + 12) + "n\0" + "c\0" + 2 */
    const Bytes all = gz10(4 | 8 | 16 | 2) + Bytes{12, 0, 'Q', 'Z', 8, 0} + le32(70000) + le32(123) + Bytes{'n', 0, 'c', 0, 1, 2};
    CHECK(hdr_is(F_GZIP_EXT, all, 30, 70000, 123));
    /* every truncation: the sizes are known once the extra field is whole, the header is an error until it all is */
    for (size_t n = 0; n < all.size(); n++) CHECK(hdr_is(F_GZIP_EXT, all, QZ_DATA_ERROR, n >= 24 ? 70000 : 0, n >= 24 ? 123 : 0, n));
    const Bytes ext = gzext(65536, 777);
    for (size_t n = 0; n < 24; n++) CHECK(hdr_is(F_GZIP_EXT, ext, QZ_DATA_ERROR, 0, 0, n));
    CHECK(hdr_is(F_GZIP_EXT, ext, 24, 65536, 777, 24));
}

/* ------------------------------------------------------------------ sized members */
/* header with both sizes, csz bytes of payload, 8 of trailer: 32 + csz bytes */
static Bytes sized(uint32_t usz, uint32_t csz) { return gzext(usz, csz) + fill(csz, 0xd0) + fill(8, 0x77); }

static uint32_t walk(const Bytes &b, size_t n, uint32_t cap, std::vector<QzSized> *mem)
{
    Exact e(b, n);
    mem->clear();
    return qz_sized_walk(e.p, e.n, cap, mem);
}
static bool sized_is(const QzSized &m, uint32_t pay, uint32_t csz, uint32_t usz) { return m.pay == pay && m.csz == csz && m.usz == usz; }

static void test_sized_walk(void)
{
    std::vector<QzSized> mem;
    /* three members: 37, 38 and 39 bytes, payloads at 24, 37 + 24, 75 + 24 */
    const Bytes m0 = sized(100, 5), m1 = sized(200, 6), m2 = sized(300, 7), three = m0 + m1 + m2;
    CHECK(three.size() == 114);
    CHECK(walk(three, 114, 600, &mem) == 114 && mem.size() == 3);
    CHECK(mem.size() == 3 && sized_is(mem[0], 24, 5, 100) && sized_is(mem[1], 61, 6, 200) && sized_is(mem[2], 99, 7, 300));
    CHECK(walk(three, 114, 0xffffffffu, &mem) == 114 && mem.size() == 3);
    /* something that is no member behind them changes nothing */
    CHECK(walk(three + fill(9, 0), 123, 600, &mem) == 114 && mem.size() == 3);
    /* not sized: a size of zero, a plain gzip header, no header at all - at member 0 and at member 2 */
    const Bytes unsized[4] = {sized(0, 7), gzext(300, 0) + fill(8, 0x77), gz10(0) + fill(20, 0), fill(30, 0xee)};
    for (int k = 0; k < 4; k++) {
        CHECK(walk(unsized[k] + m1 + m2, unsized[k].size() + 77, 600, &mem) == 0 && mem.empty());
        CHECK(walk(m0 + m1 + unsized[k], 75 + unsized[k].size(), 600, &mem) == 75 && mem.size() == 2);
    }
    /* cut short: the last trailer byte is missing; anything shorter too, down to a cut header */
    CHECK(walk(m0, 36, 600, &mem) == 0 && mem.empty());
    CHECK(walk(three, 113, 600, &mem) == 75 && mem.size() == 2);
    for (size_t n = 75; n < 114; n++) CHECK(walk(three, n, 600, &mem) == 75 && mem.size() == 2);
    for (size_t n = 0; n < 37; n++) CHECK(walk(three, n, 600, &mem) == 0 && mem.empty());
    /* destination full: whole members only */
    CHECK(walk(three, 114, 99, &mem) == 0 && mem.empty());
    CHECK(walk(three, 114, 100, &mem) == 37 && mem.size() == 1);
    CHECK(walk(three, 114, 599, &mem) == 75 && mem.size() == 2);
    /* larger than any hw_buff_sz: 512 KiB is a chunk, one byte more is not */
    CHECK(QZ_SIZED_MAX == 524288);
    CHECK(walk(sized(524289, 5) + m1 + m2, 114, 0xffffffffu, &mem) == 0 && mem.empty());
    CHECK(walk(m0 + m1 + sized(524289, 7), 114, 0xffffffffu, &mem) == 75 && mem.size() == 2);
    CHECK(walk(m0 + m1 + sized(524288, 7), 114, 0xffffffffu, &mem) == 114 && mem.size() == 3 && sized_is(mem[2], 99, 7, 524288));
    /* a single member: fewer than 2, so not this kind of stream */
    CHECK(walk(m0, 37, 600, &mem) == 37 && mem.size() == 1 && sized_is(mem[0], 24, 5, 100));
    CHECK(walk(Bytes{}, 0, 600, &mem) == 0 && mem.empty());
    /* a compressed size that would carry the position past 32 bits is cut short, not wrapped */
    CHECK(walk(m0 + gzext(10, 0xfffffff0u), 61, 600, &mem) == 37 && mem.size() == 1);
}

static bool lone(const Bytes &b, size_t n, uint32_t dest_len, uint32_t max, QzSized *m)
{
    Exact e(b, n);
    return qz_lone_sized_member(e.p, e.n, dest_len, max, m);
}

static void test_lone_member(void)
{
    QzSized m = {0, 0, 0};
    const Bytes one = sized(100, 5), more = one + fill(1, 0);
    CHECK(lone(one, 37, 100, 1000, &m) && sized_is(m, 24, 5, 100));                /* exactly the member */
    CHECK(!lone(more, 38, 100, 1000, &m));                                         /* one byte more */
    CHECK(!lone(one, 36, 100, 1000, &m));                                          /* one byte less */
    CHECK(!lone(one, 23, 100, 1000, &m) && !lone(one, 0, 100, 1000, &m));
    CHECK(lone(one, 37, 101, 1000, &m) && !lone(one, 37, 99, 1000, &m));           /* es == dest_len + 1 does not fit */
    CHECK(lone(one, 37, 1000, 100, &m) && !lone(one, 37, 1000, 99, &m));           /* es at the max, and above it */
    CHECK(!lone(sized(0, 5), 37, 100, 1000, &m) && !lone(gzext(100, 0) + fill(8, 0), 32, 100, 1000, &m));
    CHECK(!lone(gz10(0) + fill(27, 0), 37, 100, 1000, &m));
}

/* ------------------------------------------------------------------ one member as one inflate segment */
static void test_member_seg(void)
{
    qzd_infseg g; qzd_range r;
    memset(&g, 0xee, sizeof(g)); memset(&r, 0xee, sizeof(r));
    qz_member_seg(&g, &r, 0x100000010ull, 777, 0x200000000ull, 65536);
    CHECK(g.in_off == 0x100000010ull && g.in_len == 777 && g.out_off == 0x200000000ull && g.out_cap == 65536 && g.flags == 0 && g.pad == 777);
    CHECK(r.off == 0x200000000ull && r.len == 65536 && r.pad == 0);
    /* the trailer: CRC-32 A1B2C3D4, ISIZE 65536 */
    const Bytes tr = Bytes{0xD4, 0xC3, 0xB2, 0xA1} + le32(65536);
    Exact e(tr);
    const qzd_infres ok = {0, 777, 65536, 3};
    CHECK(member_ok(ok, 0xA1B2C3D4u, e.p, 777, 65536));
    qzd_infres x = ok; x.status = -1; CHECK(!member_ok(x, 0xA1B2C3D4u, e.p, 777, 65536));
    x = ok; x.out_len = 65535; CHECK(!member_ok(x, 0xA1B2C3D4u, e.p, 777, 65536));
    x = ok; x.in_used = 776; CHECK(!member_ok(x, 0xA1B2C3D4u, e.p, 777, 65536));
    CHECK(!member_ok(ok, 0xA1B2C3D5u, e.p, 777, 65536));                           /* the data's CRC is not the trailer's */
    Exact f(Bytes{0xD4, 0xC3, 0xB2, 0xA1} + le32(65537));
    CHECK(!member_ok(ok, 0xA1B2C3D4u, f.p, 777, 65536));                           /* ISIZE is not the header's size */
    x = ok; x.nblocks = 0; CHECK(member_ok(x, 0xA1B2C3D4u, e.p, 777, 65536));      /* (the block count is not part of it) */
}

/* ------------------------------------------------------------------ the LZ4 frame extent */
/* magic, FLG (version 01, the given bits), BD, [content size], [dictionary id], HC; then the caller's blocks */
enum { L_DICT = 0x01, L_CSUM = 0x04, L_CSIZE = 0x08, L_BSUM = 0x10 };
static Bytes lz4_head(unsigned bits, uint64_t content, unsigned version = 1)
{
    Bytes h = le32(0x184D2204u) + Bytes{(unsigned char)(version << 6 | 0x20 | bits), 0x40};
    if (bits & L_CSIZE) h = h + le32((uint32_t)content) + le32((uint32_t)(content >> 32));
    if (bits & L_DICT) h = h + le32(0x11223344u);
    return h + Bytes{0x5a};
}
static Bytes lz4_block(unsigned bits, uint32_t n, bool stored = false)
{ return le32(n | (stored ? 0x80000000u : 0)) + fill(n, 0xb1) + ((bits & L_BSUM) ? le32(0xcccccccc) : Bytes{}); }
static Bytes lz4_end(unsigned bits) { return le32(0) + ((bits & L_CSUM) ? le32(0xdddddddd) : Bytes{}); }

static bool extent_is(const Bytes &b, size_t n, int64_t want, bool want_hc = false, uint64_t want_content = 0)
{
    Exact e(b, n);
    uint64_t content = 0x5555, bound = 0; bool hc = false;
    const int64_t got = lz4_frame_extent(e.p, e.n, &content, &hc, &bound);
    if (bound != UINT64_MAX) { printf("  bound %llu\n", (unsigned long long)bound); return false; }
    if (got == want && (want < 0 || (hc == want_hc && content == want_content))) return true;
    printf("  got %lld (%d, %llu), want %lld (%d, %llu)\n", (long long)got, hc, (unsigned long long)content, (long long)want, want_hc, (unsigned long long)want_content);
    return false;
}

static void test_lz4_extent(void)
{
    /* without a content size: 7 of header, 4 + 5 of block, 4 of end mark */
    Bytes f = lz4_head(0, 0) + lz4_block(0, 5) + lz4_end(0);
    CHECK(f.size() == 20 && extent_is(f, 20, 20));
    CHECK(extent_is(f + fill(7, 0x33), 27, 20));                                  /* what follows the frame is not its business */
    /* with one, all 64 bits of it: 8 bytes more */
    f = lz4_head(L_CSIZE, 0x0000000100000005ull) + lz4_block(0, 5) + lz4_end(0);
    CHECK(f.size() == 28 && extent_is(f, 28, 28, true, 0x0000000100000005ull));
    CHECK(extent_is(lz4_head(L_CSIZE, 0) + lz4_end(0), 19, 19, true, 0));          /* an empty frame that says so */
    CHECK(extent_is(lz4_head(0, 0) + lz4_end(0), 11, 11));
    /* block checksums and a content checksum: 4 behind every block, 4 behind the end mark */
    f = lz4_head(L_BSUM | L_CSUM, 0) + lz4_block(L_BSUM, 5) + lz4_block(L_BSUM, 1) + lz4_end(L_CSUM);
    CHECK(f.size() == 7 + 13 + 9 + 8 && extent_is(f, 37, 37));
    /* a dictionary id: 4 more of header */
    f = lz4_head(L_DICT | L_CSIZE, 9) + lz4_block(0, 9) + lz4_end(0);
    CHECK(f.size() == 19 + 13 + 4 && extent_is(f, 36, 36, true, 9));
    /* a stored block: the high bit of its header is not part of its size */
    f = lz4_head(0, 0) + lz4_block(0, 6, true) + lz4_end(0);
    CHECK(f.size() == 21 && extent_is(f, 21, 21));
    /* two blocks, every feature, cut at every byte */
    f = lz4_head(L_CSIZE | L_BSUM | L_CSUM, 12) + lz4_block(L_BSUM, 5) + lz4_block(L_BSUM, 7, true) + lz4_end(L_CSUM);
    CHECK(f.size() == 15 + 13 + 15 + 8 && extent_is(f, 51, 51, true, 12));
    for (size_t n = 0; n < 51; n++) CHECK(extent_is(f, n, -1));
    f = lz4_head(0, 0) + lz4_block(0, 5) + lz4_block(0, 7) + lz4_end(0);
    CHECK(f.size() == 31);
    for (size_t n = 0; n < 31; n++) CHECK(extent_is(f, n, -1));
    /* a block size that reaches past the end, by one and by nearly 2^31 */
    CHECK(extent_is(lz4_head(0, 0) + le32(6) + fill(5, 0), 16, -1));
    CHECK(extent_is(lz4_head(0, 0) + le32(0x7fffffffu) + fill(5, 0), 16, -1) && extent_is(lz4_head(0, 0) + le32(0xffffffffu) + fill(5, 0), 16, -1));
    /* wrong magic (a skippable frame's too: the LZ4 session does not take them), version bits other than 01 */
    f = lz4_head(0, 0) + lz4_block(0, 5) + lz4_end(0);
    Bytes bad = f; bad[0] = 0x05; CHECK(extent_is(bad, 20, -1));
    bad = f; bad[3] = 0x19; CHECK(extent_is(bad, 20, -1));
    bad = le32(0x184D2A50u) + le32(12) + fill(12, 0); CHECK(extent_is(bad, 20, -1));
    for (unsigned v = 0; v < 4; v++) CHECK(extent_is(lz4_head(0, 0, v) + lz4_block(0, 5) + lz4_end(0), 20, v == 1 ? 20 : -1));
}

/* ------------------------------------------------------------------ the frame plan */
/* a stub codec: a frame is [length >= 4 | 0xff malformed] [has a content size] [content size] [bound, 0xff none] and filler */
static int64_t stub_extent(const uint8_t *p, uint64_t n, uint64_t *content, bool *has_content, uint64_t *bound)
{
    if (n < 4 || p[0] == 0xff || p[0] > n) return -1;
    *has_content = p[1] != 0; *content = p[2]; *bound = p[3] == 0xff ? UINT64_MAX : p[3];
    return p[0];
}
static Bytes frame(unsigned char len, unsigned char content) { return Bytes{len, 1, content, 0} + fill(len - 4, 0xf0); }
static Bytes unknown(unsigned char len, unsigned char bound) { return Bytes{len, 0, 0x99, bound} + fill(len - 4, 0xf1); }
static const Bytes k_malformed = {0xff, 1, 1, 1, 0, 0};

static int plan(const Bytes &b, uint32_t cap, QzFramePlan *pl)
{
    Exact e(b);
    pl->ti = 12345; pl->alone = true; pl->segs.resize(3);           /* whatever an earlier plan left */
    return qz_frame_plan(stub_extent, e.p, e.n, cap, pl);
}
static bool seg_is(const qzd_lz4seg &g, uint64_t in_off, uint32_t in_len, uint64_t out_off, uint32_t out_cap)
{
    if (g.in_off == in_off && g.in_len == in_len && g.out_off == out_off && g.out_cap == out_cap) return true;
    printf("  got in %llu+%u out %llu+%u\n", (unsigned long long)g.in_off, g.in_len, (unsigned long long)g.out_off, g.out_cap);
    return false;
}

static void test_frame_plan(void)
{
    QzFramePlan pl;
    const Bytes A = frame(6, 10), B = frame(4, 20), C = frame(9, 5);
    /* both rules for a frame of unknown size: the rest of cap (bound none, LZ4), or that capped by a bound (zstd) */
    for (int bounded = 0; bounded < 2; bounded++) {
        const Bytes U = unknown(7, bounded ? 30 : 0xff);
        /* all frames fit: one behind the other in both buffers */
        CHECK(plan(A + B + C, 35, &pl) == QZ_OK && pl.segs.size() == 3 && pl.ti == 19 && !pl.alone);
        CHECK(pl.segs.size() == 3 && seg_is(pl.segs[0], 0, 6, 0, 10) && seg_is(pl.segs[1], 6, 4, 10, 20) && seg_is(pl.segs[2], 10, 9, 30, 5));
        CHECK(plan(A + B + C, 1000, &pl) == QZ_OK && pl.segs.size() == 3 && pl.ti == 19 && !pl.alone);
        /* the first frame malformed, or cut */
        CHECK(plan(k_malformed + A, 100, &pl) == QZ_FAIL && pl.segs.empty());
        CHECK(plan(Bytes{6, 1, 10, 0, 0}, 100, &pl) == QZ_FAIL && plan(Bytes{6, 1, 10}, 100, &pl) == QZ_FAIL);
        /* the second: the plan is the first frame */
        CHECK(plan(A + k_malformed + C, 100, &pl) == QZ_OK && pl.segs.size() == 1 && pl.ti == 6 && !pl.alone && seg_is(pl.segs[0], 0, 6, 0, 10));
        CHECK(plan(A + Bytes{4, 1, 20}, 100, &pl) == QZ_OK && pl.segs.size() == 1 && pl.ti == 6 && !pl.alone);
        /* the first frame too big, by one byte */
        CHECK(plan(A + B, 9, &pl) == QZ_BUF_ERROR && pl.segs.empty());
        CHECK(plan(A + B, 10, &pl) == QZ_OK && pl.segs.size() == 1 && pl.ti == 6);
        /* the second too big: the first only */
        CHECK(plan(A + B + C, 29, &pl) == QZ_OK && pl.segs.size() == 1 && pl.ti == 6 && !pl.alone);
        CHECK(plan(A + B + C, 30, &pl) == QZ_OK && pl.segs.size() == 2 && pl.ti == 10 && !pl.alone);      /* cap == to behind B: C is not looked at */
        CHECK(plan(A + B + k_malformed, 30, &pl) == QZ_OK && pl.segs.size() == 2 && pl.ti == 10);
        CHECK(plan(A + B + C, 34, &pl) == QZ_OK && pl.segs.size() == 2 && pl.ti == 10);
        /* a frame of unknown size mid-stream gets what is left by its rule, ends the plan behind it, and is marked alone */
        CHECK(plan(A + U + C, 100, &pl) == QZ_OK && pl.segs.size() == 2 && pl.ti == 13 && pl.alone);
        CHECK(pl.segs.size() == 2 && seg_is(pl.segs[0], 0, 6, 0, 10) && seg_is(pl.segs[1], 6, 7, 10, bounded ? 30 : 90));
        CHECK(plan(A + U + C, 25, &pl) == QZ_OK && pl.segs.size() == 2 && pl.alone && seg_is(pl.segs[1], 6, 7, 10, 15));   /* the bound is above what is left */
        CHECK(plan(A + U + C, 40, &pl) == QZ_OK && pl.segs.size() == 2 && pl.alone && seg_is(pl.segs[1], 6, 7, 10, 30));   /* at it */
        CHECK(plan(A + U + C, 41, &pl) == QZ_OK && pl.segs.size() == 2 && pl.alone && seg_is(pl.segs[1], 6, 7, 10, bounded ? 30 : 31));
        /* ... as the first frame too: it is never too big */
        CHECK(plan(U + A, 1, &pl) == QZ_OK && pl.segs.size() == 1 && pl.ti == 7 && pl.alone && seg_is(pl.segs[0], 0, 7, 0, 1));
        CHECK(plan(U + A, 64, &pl) == QZ_OK && pl.segs.size() == 1 && pl.ti == 7 && pl.alone && seg_is(pl.segs[0], 0, 7, 0, bounded ? 30 : 64));
        /* cap == to after a frame stops the plan; an unknown one behind it is not begun with nothing */
        CHECK(plan(A + U, 10, &pl) == QZ_OK && pl.segs.size() == 1 && pl.ti == 6 && !pl.alone);
        CHECK(plan(A + frame(4, 0), 10, &pl) == QZ_OK && pl.segs.size() == 1 && pl.ti == 6);
        CHECK(plan(A + frame(4, 0) + B, 30, &pl) == QZ_OK && pl.segs.size() == 3 && pl.ti == 14 && seg_is(pl.segs[1], 6, 4, 10, 0) && seg_is(pl.segs[2], 10, 4, 10, 20));
        /* nothing to read, nowhere to write: an empty plan, and that is no error */
        CHECK(plan(Bytes{}, 100, &pl) == QZ_OK && pl.segs.empty() && pl.ti == 0 && !pl.alone);
        CHECK(plan(A + B, 0, &pl) == QZ_OK && pl.segs.empty() && pl.ti == 0 && !pl.alone);
        CHECK(plan(k_malformed, 0, &pl) == QZ_OK && pl.segs.empty());
    }
    /* a zstd bound of 0 (a frame of skippable or empty blocks only): a segment of no output, still alone */
    CHECK(plan(A + unknown(5, 0) + C, 100, &pl) == QZ_OK && pl.segs.size() == 2 && pl.alone && pl.ti == 11 && seg_is(pl.segs[1], 6, 5, 10, 0));
}

/* ------------------------------------------------------------------ the result check */
static void test_frames_produced(void)
{
    static const qzd_lz4seg segs[3] = {{0, 0, 6, 10}, {6, 10, 4, 20}, {10, 30, 9, 50}};
    static const qzd_lz4res exact[3] = {{0, 6, 10, 0}, {0, 4, 20, 0}, {0, 9, 50, 0}};
    static const QzShortRule rules[2] = {QZ_SHORT_LAST, QZ_SHORT_LAST_UNSIZED};
    for (int k = 0; k < 2; k++) for (int alone = 0; alone < 2; alone++) {
        const QzShortRule rule = rules[k];
        /* LZ4: the last segment may come short, sized or not.  zstd: only an unsized last one */
        const bool last_may = rule == QZ_SHORT_LAST || alone;
        qzd_lz4res r[3];
        memcpy(r, exact, sizeof(r));
        CHECK(qz_frames_produced(segs, r, 3, alone, rule) == 80);                 /* all exact: 30 + 50 */
        CHECK(qz_frames_produced(segs, r, 2, alone, rule) == 30 && qz_frames_produced(segs, r, 1, alone, rule) == 10);
        CHECK(qz_frames_produced(segs, r, 0, alone, rule) == 0);
        r[2].out_len = 49;                                                        /* the last one short */
        CHECK(qz_frames_produced(segs, r, 3, alone, rule) == (last_may ? 79 : -1));
        r[2].out_len = 0;
        CHECK(qz_frames_produced(segs, r, 3, alone, rule) == (last_may ? 30 : -1));
        memcpy(r, exact, sizeof(r)); r[1].out_len = 19;                           /* a middle one short: never */
        CHECK(qz_frames_produced(segs, r, 3, alone, rule) == -1);
        CHECK(qz_frames_produced(segs, r, 2, alone, rule) == (last_may ? 29 : -1));    /* (as the last of two it is the last) */
        memcpy(r, exact, sizeof(r)); r[0].out_len = 9;
        CHECK(qz_frames_produced(segs, r, 3, alone, rule) == -1);
        CHECK(qz_frames_produced(segs, r, 1, alone, rule) == (last_may ? 9 : -1));
        for (int i = 0; i < 3; i++) {
            memcpy(r, exact, sizeof(r)); r[i].status = -1;                        /* a frame that failed, wherever */
            CHECK(qz_frames_produced(segs, r, 3, alone, rule) == -1);
            memcpy(r, exact, sizeof(r)); r[i].in_used = segs[i].in_len - 1;        /* input left over */
            CHECK(qz_frames_produced(segs, r, 3, alone, rule) == -1);
            memcpy(r, exact, sizeof(r)); r[i].in_used = segs[i].in_len + 1;
            CHECK(qz_frames_produced(segs, r, 3, alone, rule) == -1);
        }
        memcpy(r, exact, sizeof(r)); r[2].out_len = 49; r[2].status = -2;          /* short AND failed is failed */
        CHECK(qz_frames_produced(segs, r, 3, alone, rule) == -1);
    }
}

/* ------------------------------------------------------------------ the crc out-parameter */
/* zlib's crc32_combine, bit by bit: crc1's register goes through 8 * len2 zero bits of the reflected CRC-32, crc2 is added */
static uint32_t combine_bits(uint32_t crc1, uint32_t crc2, uint64_t len2)
{
    for (uint64_t i = 0; i < 8 * len2; i++) crc1 = (crc1 >> 1) ^ ((crc1 & 1) ? 0xEDB88320u : 0);
    return crc1 ^ crc2;
}
/* the combine the header links against (the library's is in the device layer) */
extern "C" uint32_t qzd_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) { return combine_bits(crc1, crc2, len2); }

static void test_fold(void)
{
    /* the combine itself on a known pair: crc32("123456789") = cbf43926, crc32("12345") = cbf53a1c, crc32("6789") = 9dbabf87 */
    CHECK(combine_bits(0xcbf53a1cu, 0x9dbabf87u, 4) == 0xcbf43926u);
    const uint32_t c = 0x2468ACE0u, X = 0x0BADF00Du, len = 1000;
    unsigned long crc;
    /* a member of a call: taken only by a *crc of 0 at the call's first output.  (Combining onto 0 gives c as well - a CRC of
     * nothing shifted is nothing - so the three rules differ in what they compute, not in what comes out) */
    crc = 0; qz_crc_fold_member(&crc, 0, c, len); CHECK(crc == c);
    crc = 0; qz_crc_fold_member(&crc, 4096, c, len); CHECK(crc == combine_bits(0, c, len));
    crc = X; qz_crc_fold_member(&crc, 0, c, len); CHECK(crc == combine_bits(X, c, len));
    crc = X; qz_crc_fold_member(&crc, 4096, c, len); CHECK(crc == combine_bits(X, c, len));
    /* a call's only output: a *crc of 0 takes */
    crc = 0; qz_crc_fold_lone(&crc, c, len); CHECK(crc == c);
    crc = X; qz_crc_fold_lone(&crc, c, len); CHECK(crc == combine_bits(X, c, len));
    /* a later piece: always combined */
    crc = 0; qz_crc_fold_piece(&crc, c, len); CHECK(crc == combine_bits(0, c, len));
    crc = X; qz_crc_fold_piece(&crc, c, len); CHECK(crc == combine_bits(X, c, len));
    /* only the low 32 bits of the out-parameter are a CRC */
    crc = (unsigned long)0xffffffff00000000ull | X; qz_crc_fold_piece(&crc, c, len); CHECK(crc == combine_bits(X, c, len));
}

int main(void)
{
    test_header();
    test_sized_walk();
    test_lone_member();
    test_member_seg();
    test_lz4_extent();
    test_frame_plan();
    test_frames_produced();
    test_fold();
    if (g_fail) { printf("qz_unframe_test: %d FAILED\n", g_fail); return 1; }
    printf("qz_unframe_test: ok\n");
    return 0;
}
