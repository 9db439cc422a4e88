"""Block-addressable compression on the GPU: the programmable CRC and XXH32 of ranges through the device layer
(qzd_crcn_ranges / qzd_xxh32_ranges), qzCompressWithMetadataExt / qzDecompressWithMetadataExt against the CPU oracle's raw
deflate of every block, the metadata records against tests/crcmodel.py and the oracle's XXH32, and the Crc64 calls.
The emulator twin of the kernel cases is tests/test_sim_meta.py; the blob's own rules are in tests/test_meta_blob.py."""
import ctypes as C
import zlib

import numpy as np
import pytest

import crcmodel
import datagen
import oracle_lib as O
from qatzip_amd import api as A
from qatzip_amd import _lib

pytestmark = pytest.mark.gpu

QZD_ERR_DSTCAP, QZD_ERR_DATA = -3, -4
CRC_LENS = (0, 1, 7, 8, 9, 255, 256, 257, 4095, 65536, 65537)
KINDS = ("text", "rand", "silesia", "runs")
SESSION_B = 8192                      # the session's own hw_buff_sz: what override 0 selects


@pytest.fixture(scope="module")
def ctx():
    import qatzip_amd
    c = qatzip_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def buf():
    return datagen.gen_bytes("text", 40000, 5) + datagen.gen_bytes("rand", 100000, 6) + datagen.gen_bytes("silesia", (1 << 20) + 3, 7)


@pytest.fixture(scope="module")
def d_buf(ctx, buf):
    d = ctx.alloc(len(buf))
    d.upload(buf)
    yield d
    d.free()


def xxh(b):
    return O.lib().qzo_xxh32(b, len(b), 0)


# ------------------------------------------------------------------ kernels through the device layer
@pytest.mark.parametrize("name", sorted(crcmodel.CATALOGUE))
def test_crcn_ranges_match_the_model(ctx, buf, d_buf, name):
    cfg, check = crcmodel.CATALOGUE[name]
    d9 = ctx.alloc(16); d9.upload(b"123456789")
    assert [int(v) for v in ctx.crcn_ranges(d9, [(0, 9)], cfg[0], cfg[1:])] == [check]
    d9.free()
    ranges, off = [], 1
    for n in CRC_LENS:
        ranges.append((off, n))
        off = (off + n // 3 + 2) | 1
    big = (139999, (1 << 20) + 3)                               # one long range: 4 KiB slices, tails past 2^20
    ranges.append(big)
    assert all(o + n <= len(buf) for o, n in ranges)
    got = ctx.crcn_ranges(d_buf, ranges, cfg[0], cfg[1:])
    for (o, n), g in zip(ranges, got):
        assert int(g) == crcmodel.crc_fast(cfg, buf[o:o + n]), (name, o, n)
    ranges = [(1001 + 2 * i, n) for i, n in enumerate(CRC_LENS)]
    start = [crcmodel.crc_fast(cfg, buf[o - 1000:o]) for o, _ in ranges]
    start[3] = crcmodel.empty(cfg)
    got = ctx.crcn_ranges(d_buf, ranges, cfg[0], cfg[1:], start)
    for i, ((o, n), g) in enumerate(zip(ranges, got)):
        want = crcmodel.crc_fast(cfg, buf[o:o + n]) if i == 3 else crcmodel.crc_fast(cfg, buf[o - 1000:o + n])
        assert int(g) == want, (name, o, n)


def test_crcn_ranges_refuses_what_is_no_config(ctx, d_buf):
    L = ctx.L
    out = np.zeros(1, np.uint64); ra = np.array([(0, 9, 0)], dtype=_lib.RANGE_DT)
    for width, cfg in ((16, (0x1021, 0, 0, 0, 0)), (32, (0x04C11DB6, 0, 0, 0, 0)), (32, (0x104C11DB7, 0, 0, 0, 0)),
                       (64, (0x1B, 0, 2, 0, 0)), (64, (0x1B, 0, 0, 3, 0))):
        assert L.qzd_crcn_ranges(ctx.h, d_buf.ptr, ra.ctypes.data, 1, width, C.byref(_lib.CrcCfg(*cfg)), None, out.ctypes.data) == -1


def test_xxh32_ranges_match_the_oracle(ctx, buf, d_buf):
    ranges, off = [], 3
    for n in (0, 15, 16, 17, 2047, 2048, 65536, (1 << 20) + 3):
        ranges.append((off, n))
        off += min(n, 70000) // 2 + 5
    got = ctx.xxh32_ranges(d_buf, ranges)
    for (o, n), g in zip(ranges, got):
        assert int(g) == xxh(buf[o:o + n]), (o, n)


# ------------------------------------------------------------------ compress / decompress with metadata
def raw_session(lvl=1, hw=SESSION_B):
    s = A.Session(A.QZ_DEFLATE_RAW, hw_buff_sz=hw, comp_lvl=lvl)
    assert s.rc_setup == A.QZ_OK
    return s


def oracle_blocks(src, B, lvl):
    return [O.sw_compress("RAW", src[o:o + B], B, lvl)[2] for o in range(0, len(src), B)]


def check_blocks(s, src, B, lvl, thr, override, cfg32=crcmodel.CRC32_ISO_HDLC, cfg64=crcmodel.CRC64_ECMA, tag=None):
    """one qzCompressWithMetadataExt call checked block by block, then the round trip -> (records, compressed bytes)"""
    n = len(src)
    nb = (n + B - 1) // B
    meta = A.Metadata(n, B)
    assert meta.rc_alloc == A.QZ_OK
    rc, used, comp = s.compress_meta(src, meta, thr, override=override)
    assert (rc, used) == (A.QZ_OK, n), (tag, rc, used)
    streams = oracle_blocks(src, B, lvl)
    pos, recs, plains, outs = 0, [], [], []
    for k in range(nb):
        plain = src[k * B:(k + 1) * B]
        rrc, off, size, flags, h = meta.read(k)
        assert rrc == A.QZ_OK and off == pos, (tag, k, off, pos)                # back to back from 0
        keep = len(streams[k]) <= thr
        assert flags == (1 if keep else 0), (tag, k, len(streams[k]), thr)
        got = comp[off:off + size]
        if keep:
            assert got == streams[k], (tag, k)                                  # byte for byte the oracle's raw deflate of the block
            assert zlib.decompress(got, -15) == plain, (tag, k)
        else:
            assert size == len(plain) and got == plain, (tag, k)
        assert h == xxh(plain), (tag, k)
        recs.append((off, size, flags, h)); plains.append(plain); outs.append(got)
        pos += size
    assert pos == len(comp), tag
    i32, o32 = crcmodel.crc_many(cfg32, plains), crcmodel.crc_many(cfg32, outs)
    i64, o64 = crcmodel.crc_many(cfg64, plains), crcmodel.crc_many(cfg64, outs)
    for k in range(nb):
        assert meta.crc32(k) == (A.QZ_OK, i32[k], o32[k]), (tag, k)
        assert meta.crc64(k) == (A.QZ_OK, i64[k], o64[k]), (tag, k)
    rc, used, back = s.decompress_meta(comp, meta, n, override=override)
    assert (rc, used) == (A.QZ_OK, len(comp)) and back == src, (tag, rc, used, len(back))
    assert [meta.read(k)[1:] for k in range(nb)] == recs                        # decompress leaves the blob alone
    assert meta.free() == A.QZ_OK
    return recs, comp


def sizes_for(B):
    return [1, B - 1, B, B + 1, 3 * B + 1234] + ([1100 * 1024] if B == 1024 else [])


@pytest.mark.parametrize("B", [1024, 65536, 0])
@pytest.mark.parametrize("lvl", [1, 6, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_compress_with_metadata_block_by_block(kind, lvl, B):
    """B = 0: the session's hw_buff_sz through override 0.  thr = B: a block is kept compressed when that does not grow it
    (every block of `rand` is stored)"""
    s = raw_session(lvl)
    bsz = B or SESSION_B
    for n in sizes_for(bsz):
        src = datagen.gen_bytes(kind, n, 31 + lvl)
        recs, _ = check_blocks(s, src, bsz, lvl, bsz, B, tag=(kind, lvl, bsz, n))
        if kind == "rand":                                      # (a short last block whose stream is within thr stays compressed)
            assert all(f == 0 for k, (_, _, f, _) in enumerate(recs) if n - k * bsz >= bsz - 1), (lvl, bsz, n)
        if kind in ("text", "runs") and n >= bsz:
            assert any(f == 1 for _, _, f, _ in recs), (kind, lvl, bsz, n)
    s.close()


def test_records_under_other_crc_configs():
    """the records' CRCs follow the session's configs (XZ and CRC-32C here); the gzip CRC-32 of the wire formats does not"""
    s = raw_session(1)
    assert s.set_crc64(*crcmodel.CRC64_XZ[1:]) == A.QZ_OK and s.set_crc32(*crcmodel.CRC32C[1:]) == A.QZ_OK
    for kind in KINDS:
        src = datagen.gen_bytes(kind, 40 * 1024 + 77, 3)
        check_blocks(s, src, 1024, 1, 1024, 1024, cfg32=crcmodel.CRC32C, cfg64=crcmodel.CRC64_XZ, tag=kind)
    src = datagen.gen_bytes("text", 70000, 4)
    rc, used, out, crc = s.compress(src, crc0=0)
    assert rc == A.QZ_OK and crc == zlib.crc32(src)                             # qzCompressCrc's crc stays zlib's
    s.close()


def test_threshold_edge_and_threshold_zero():
    B = 1024
    src = datagen.gen_bytes("text", 4 * B, 12)
    s = raw_session(1)
    c = len(oracle_blocks(src, B, 1)[2])
    assert 0 < c < B
    for thr, want in ((c, (1, c)), (c - 1, (0, B))):
        meta = A.Metadata(len(src), B)
        rc, used, comp = s.compress_meta(src, meta, thr, override=B)
        assert rc == A.QZ_OK and used == len(src)
        _, _, size, flags, _ = meta.read(2)
        assert (flags, size) == want, (thr, flags, size)
        assert s.decompress_meta(comp, meta, len(src), override=B)[2] == src
        meta.free()
    meta = A.Metadata(len(src), B)                                              # the header read literally: threshold 0 stores everything
    rc, used, comp = s.compress_meta(src, meta, 0, override=B)
    assert rc == A.QZ_OK and comp == src and all(meta.read(k)[2:4] == (B, 0) for k in range(4))
    meta.free()
    s.close()


def test_overflow_short_destination_formats_and_bad_override():
    B = 1024
    src = datagen.gen_bytes("text", 10 * B + 5, 8)
    s = raw_session(1)
    small = A.Metadata(10 * B, B)                                               # ten records, eleven blocks
    rc, used, comp = s.compress_meta(src, small, B, override=B)
    assert (rc, used, comp) == (A.QZ_METADATA_OVERFLOW, 0, b"")
    assert small.read(0) == (A.QZ_OK, 0, 0, 0, 0)
    small.free()
    meta = A.Metadata(len(src), B)
    rc, used, full = s.compress_meta(src, meta, B, override=B)
    assert rc == A.QZ_OK
    ends = [meta.read(k)[1] + meta.read(k)[2] for k in range(11)]
    part = A.Metadata(len(src), B)
    rc, used, comp = s.compress_meta(src, part, B, override=B, cap=ends[4] + 3)  # five whole blocks and a bit
    assert (rc, used) == (A.QZ_BUF_ERROR, 5 * B) and comp == full[:ends[4]]
    assert [part.read(k) for k in range(5)] == [meta.read(k) for k in range(5)] and part.read(5) == (A.QZ_OK, 0, 0, 0, 0)
    rc, used, back = s.decompress_meta(comp, part, 5 * B, override=B)           # what was taken decodes on its own
    assert (rc, used) == (A.QZ_OK, len(comp)) and back == src[:5 * B]
    rc, used, comp = s.compress_meta(src, part, B, override=B, cap=ends[0] - 1)  # not even one block
    assert (rc, used, comp) == (A.QZ_BUF_ERROR, 0, b"")
    rc, used, comp = s.compress_meta(b"", part, B, override=B)
    assert (rc, used, comp) == (A.QZ_OK, 0, b"")
    for bad in (1000, 512, 1024 * 1024, 3 * 1024):
        assert s.compress_meta(src, meta, B, override=bad)[0] == A.QZ_PARAMS, bad
        assert s.decompress_meta(full, meta, len(src), override=bad)[0] == A.QZ_PARAMS, bad
    assert s.compress_meta(src, meta, B, override=B, last=2)[0] == A.QZ_PARAMS
    for other in (A.Session(A.QZ_DEFLATE_GZIP_EXT, hw_buff_sz=B), A.Session(hw_buff_sz=B, lz4=True)):
        assert other.rc_setup == A.QZ_OK
        assert other.compress_meta(src, meta, B, override=B)[0] == A.QZ_NOT_SUPPORTED
        assert other.decompress_meta(full, meta, len(src), override=B)[0] == A.QZ_NOT_SUPPORTED
        other.close()
    part.free(); meta.free()
    s.close()


def test_one_block_through_a_one_record_blob_and_damage():
    B = 1024
    src = datagen.gen_bytes("text", 6 * B, 21) + datagen.gen_bytes("rand", 2 * B + 100, 22)   # compressed blocks, then stored ones
    s = raw_session(6)
    meta = A.Metadata(len(src), B)
    rc, used, comp = s.compress_meta(src, meta, B, override=B)
    assert rc == A.QZ_OK
    recs = [meta.read(k)[1:] for k in range(9)]
    assert recs[3][2] == 1 and recs[7][2] == 0
    for k in (3, 7):                                                            # random access: a compressed and a stored block
        one = A.Metadata(B, B)
        off, size, flags, h = recs[k]
        assert one.write(0, offset=off, size=size, flags=flags, hash=h) == A.QZ_OK
        rc, used, out = s.decompress_meta(comp, one, B, override=B)
        assert (rc, used, out) == (A.QZ_OK, off + size, src[k * B:(k + 1) * B]), k
        one.free()
    # a short destination: all or nothing
    assert s.decompress_meta(comp, meta, len(src) - 1, override=B) == (A.QZ_BUF_ERROR, 0, b"")
    assert s.decompress_meta(comp, meta, 3 * B, override=B) == (A.QZ_BUF_ERROR, 0, b"")
    # a flipped byte in a compressed block, in a stored block, in a record's hash; a block cut off by src_len
    for at in (recs[3][0] + recs[3][1] // 2, recs[7][0] + 10):
        bad = bytearray(comp); bad[at] ^= 0x10
        assert s.decompress_meta(bytes(bad), meta, len(src), override=B) == (A.QZ_DATA_ERROR, 0, b""), at
    assert meta.write(5, hash=recs[5][3] ^ 1) == A.QZ_OK
    assert s.decompress_meta(comp, meta, len(src), override=B) == (A.QZ_DATA_ERROR, 0, b"")
    assert meta.write(5, hash=recs[5][3]) == A.QZ_OK
    assert s.decompress_meta(comp[:-1], meta, len(src), override=B) == (A.QZ_DATA_ERROR, 0, b"")
    rc, used, out = s.decompress_meta(comp, meta, len(src), override=B)         # and the session is none the worse for it
    assert (rc, used) == (A.QZ_OK, len(comp)) and out == src
    meta.free()
    s.close()


def test_round_trip_of_64_mib_at_64_kib_blocks():
    B, n = 65536, 64 << 20
    piece = datagen.gen("text", 1 << 20, 2)
    a = np.tile(piece, 64)
    a[::4099] ^= np.arange(len(a[::4099]), dtype=np.uint32).astype(np.uint8)    # no two blocks alike
    a[40 * B:42 * B] = datagen.gen("rand", 2 * B, 9)                            # two blocks that are stored
    src = a.tobytes()
    s = raw_session(1, hw=B)
    meta = A.Metadata(n, B)
    rc, used, comp = s.compress_meta(src, meta, B)
    assert (rc, used) == (A.QZ_OK, n) and s.last_ext_rc == 0
    flags = [meta.read(k)[3] for k in range(1024)]
    assert flags[40] == 0 and flags[41] == 0 and sum(flags) == 1022
    k = 777
    _, off, size, _, h = meta.read(k)
    assert zlib.decompress(comp[off:off + size], -15) == src[k * B:(k + 1) * B] and h == xxh(src[k * B:(k + 1) * B])
    rc, used, back = s.decompress_meta(comp, meta, n)
    assert (rc, used) == (A.QZ_OK, len(comp)) and back == src
    meta.free()
    s.close()


def test_device_layer_short_destination_and_exact_output_capacity(ctx):
    """qzd_blocks_compress with a destination that holds only some blocks writes those and nothing behind them;
    qzd_blocks_decompress needs no byte more than the output"""
    B, n = 1024, 300 * 1024 + 1                                                 # more blocks than a wave has lanes; a 1-byte last block
    src = datagen.gen_bytes("text", n, 17)
    nb = (n + B - 1) // B
    d_src = ctx.alloc(nb * B); d_src.upload(src)
    d_dst = ctx.alloc(n + 4096)
    rc, total, recs = ctx.blocks_compress(d_src, n, B, 1, B, d_dst)
    assert rc == 0 and total == int(recs["offset"][-1]) + int(recs["size"][-1])
    full = d_dst.download(total).tobytes()
    streams = oracle_blocks(src, B, 1)
    for k in (0, 63, 64, 255, 256, nb - 1):
        o, z = int(recs["offset"][k]), int(recs["size"][k])
        assert recs["flags"][k] == 1 and full[o:o + z] == streams[k], k
    assert [int(v) for v in recs["in_crc32"][:5]] == [zlib.crc32(src[k * B:(k + 1) * B]) for k in range(5)]
    cap = int(recs["offset"][200]) + 7
    d_dst.upload(b"\xEE" * (n + 4096))
    rc2, part, recs2 = ctx.blocks_compress(d_src, n, B, 1, B, d_dst, dst_cap=cap)
    assert rc2 == QZD_ERR_DSTCAP and part == int(recs["offset"][200])
    got = d_dst.download(cap + 64).tobytes()
    assert got[:part] == full[:part] and got[part:] == b"\xEE" * (cap + 64 - part)
    assert (recs2["offset"] == recs["offset"]).all() and (recs2["size"] == recs["size"]).all() and (recs2["hash"] == recs["hash"]).all()
    assert (recs2["out_crc64"][:200] == recs["out_crc64"][:200]).all()
    d_dst.upload(full)
    d_out = ctx.alloc(n)
    rc, produced, status = ctx.blocks_decompress(d_dst, total, recs, B, d_out, out_cap=n)
    assert rc == 0 and produced == n and (status == 0).all() and d_out.download(n).tobytes() == src
    rc, produced, status = ctx.blocks_decompress(d_dst, total, recs, B, d_out, out_cap=n - 1)
    assert rc == QZD_ERR_DSTCAP
    bad = recs.copy(); bad["size"][9] -= 1                                      # a stream that does not end where its record says
    rc, produced, status = ctx.blocks_decompress(d_dst, total, bad, B, d_out, out_cap=n)
    assert rc == QZD_ERR_DATA and status[9] == -1 and (np.delete(status, 9) == 0).all()
    for b in (d_src, d_dst, d_out):
        b.free()


# ------------------------------------------------------------------ the Crc64 calls
@pytest.mark.parametrize("cfg", [crcmodel.CRC64_ECMA, crcmodel.CRC64_XZ], ids=["ecma", "xz"])
def test_crc64_calls(cfg):
    src = datagen.gen_bytes("text", 300000, 14)
    for mk in (lambda: A.Session(A.QZ_DEFLATE_GZIP_EXT), lambda: A.Session(A.QZ_DEFLATE_RAW), lambda: A.Session(lz4=True)):
        plain, s = mk(), mk()
        if cfg is not crcmodel.CRC64_ECMA:
            assert s.set_crc64(*cfg[1:]) == A.QZ_OK and s.get_crc64() == (A.QZ_OK, cfg[1:])
        want = plain.compress(src)
        assert want[0] == A.QZ_OK
        rc, used, comp, crc = s.compress_crc64(src, crc0=crcmodel.empty(cfg))
        assert (rc, used, comp) == (A.QZ_OK, len(src), want[2])                 # the bytes qzCompress gives
        assert crc == crcmodel.crc_fast(cfg, src)
        # chained over two calls: the second starts from the first's CRC
        cut = 131072
        rc, used, c1, crc1 = s.compress_crc64(src[:cut], crc0=crcmodel.empty(cfg))
        assert rc == A.QZ_OK and crc1 == crcmodel.crc_fast(cfg, src[:cut])
        rc, used, c2, crc2 = s.compress_crc64(src[cut:], crc0=crc1)
        assert rc == A.QZ_OK and crc2 == crc
        rc, used, out, dcrc = s.decompress_crc64(comp, len(src), crc0=crcmodel.empty(cfg))
        assert (rc, used, out) == (A.QZ_OK, len(comp), src) and dcrc == crc     # the CRC of the output
        rc, used, out, dcrc = s.decompress_crc64(c2, len(src), crc0=crc1)       # and it chains the same way
        assert rc == A.QZ_OK and out == src[cut:] and dcrc == crc
        # on failure *crc is untouched
        rc, used, out, dcrc = s.decompress_crc64(b"\x00\x01\x02\x03" * 8, 1000, crc0=0x1234)
        assert rc < 0 and dcrc == 0x1234
        plain.close(); s.close()


def test_set_crc_config_on_a_session_never_set_up():
    L = A.lib()
    s = A.QzSession()
    g = A.QzCrc64Config(*crcmodel.CRC64_XZ[1:])
    assert L.qzSetSessionCrc64Config(C.byref(s), C.byref(g)) == A.QZ_FAIL
