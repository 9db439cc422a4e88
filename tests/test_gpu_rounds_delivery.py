"""The host code around the wave-per-chunk compressors, on the GPU.

Rounds: a call of more than 16384 chunks (4096 blocks for LZ4-HC) is worked off in rounds that share the slot buffer; chunks
are independent, so the call's output is the concatenation of two calls split at the round boundary - each a one-round call
- whatever the kernels wrote.  Delivery: a destination that holds only some of a call's chunks gets the leading ones that
fit whole, QZ_BUF_ERROR, and *src_len / *dest_len say how far it came - path by path, against the call with ample room."""
import ctypes as C

import numpy as np
import pytest

import datagen
import lz4s_format
import oracle_lib as O
import qatzip_amd
import zstd_format
import zstd_sim
from qatzip_amd import api as A
from qatzip_amd._lib import lz4s_bound, zstd_bound

pytestmark = pytest.mark.gpu

CH = 1024


@pytest.fixture(scope="module")
def ctx():
    c = qatzip_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiled():
    """300 KB of the tests' generator, tiled to 16385 chunks of 1 KB and five bytes"""
    base = np.concatenate([datagen.gen("silesia", 200000, 71), datagen.gen("text", 100000 + 37, 72)])
    n = 16385 * CH + 5
    return np.tile(base, n // base.size + 1)[:n].copy()


def _run(ctx, call, src, bound):
    d_src = ctx.alloc(src.size); d_src.upload(src)
    d_dst = ctx.alloc(bound + 64)
    n, lens = call(d_src, src.size, d_dst)
    out = d_dst.download(n).tobytes()
    d_src.free(); d_dst.free()
    return out, [int(x) for x in lens]


def _two_rounds(ctx, call, src, cut, bound, decode):
    """the call on all of src against the calls on src[:cut] and src[cut:]; decode(item, plaintext) checks one item"""
    whole, lens = _run(ctx, call, src, bound(src.size))
    head, hl = _run(ctx, call, src[:cut], bound(cut))
    tail, tl = _run(ctx, call, src[cut:], bound(src.size - cut))
    assert sum(lens) == len(whole) and lens == hl + tl
    assert whole == head + tail
    offs = np.concatenate([[0], np.cumsum(lens)])
    nfirst = len(hl)
    for i in (0, nfirst - 1, nfirst, len(lens) - 1):                # the first item, both sides of the boundary, the last
        decode(whole[offs[i]:offs[i + 1]], src[i * CH:(i + 1) * CH].tobytes())
    return lens


def test_lz4_frames_in_two_rounds(ctx, tiled):
    def decode(frame, plain):
        rc, used, back = O.sw_decompress("LZ4", frame, len(plain) + 64)
        assert rc == 0 and used == len(frame) and back == plain
    lens = _two_rounds(ctx, lambda s, n, d: ctx.lz4_compress_frames(s, n, d, CH), tiled, 16384 * CH,
                       lambda n: n + ((n + CH - 1) // CH) * 64, decode)
    assert len(lens) == 16386


def test_lz4hc_frames_in_two_rounds(ctx, tiled):
    def decode(frame, plain):
        rc, used, back = O.sw_decompress("LZ4", frame, len(plain) + 64)
        assert rc == 0 and used == len(frame) and back == plain
    src = tiled[:4097 * CH + 5]
    lens = _two_rounds(ctx, lambda s, n, d: ctx.lz4_compress_frames(s, n, d, CH, level=3), src, 4096 * CH,
                       lambda n: n + ((n + CH - 1) // CH) * 64, decode)
    assert len(lens) == 4098


def test_lz4s_blocks_in_two_rounds(ctx, tiled):
    def decode(block, plain):
        assert lz4s_format.decode(block, 3, CH) == plain
    lens = _two_rounds(ctx, lambda s, n, d: ctx.lz4s_compress_blocks(s, n, d, CH), tiled, 16384 * CH,
                       lambda n: lz4s_bound(n, CH), decode)
    assert len(lens) == 16386


def test_zstd_frames_in_two_rounds(ctx, tiled):
    def decode(frame, plain):
        assert zstd_format.decode(frame, CH) == plain
    lens = _two_rounds(ctx, lambda s, n, d: ctx.zstd_compress_frames(s, n, d, CH), tiled, 16384 * CH,
                       lambda n: zstd_bound(n, CH), decode)
    assert len(lens) == 16386


def test_zstd_encode_frames_in_two_rounds(ctx):
    """16385 frames of one record each (made in a few milliseconds): four literals that differ from frame to frame and a
    match of five"""
    frames = [zstd_sim.one_match(bytes([i & 0xff, i >> 8, 7, 9]), 5, 1) for i in range(16385)]

    def encode(fr):
        lits, seqs, desc = zstd_sim.pack_frames(fr)
        d_l = ctx.alloc(len(lits) + 16); d_l.upload(lits + b"\0")
        d_s = ctx.alloc(seqs.nbytes + 16); d_s.upload(np.concatenate([seqs, np.zeros(3, np.uint32)]).tobytes())
        cap = sum(f[0] + 12 for f in fr)
        d_dst = ctx.alloc(cap + 64)
        rc, n, lens = ctx.zstd_encode_frames(d_l, d_s, desc, d_dst, dst_cap=cap)
        out = d_dst.download(n).tobytes() if n else b""
        d_l.free(); d_s.free(); d_dst.free()
        assert rc == 0
        return out, [int(x) for x in lens]
    whole, lens = encode(frames)
    head, hl = encode(frames[:16384])
    tail, tl = encode(frames[16384:])
    assert sum(lens) == len(whole) and lens == hl + tl and whole == head + tail
    offs = np.concatenate([[0], np.cumsum(lens)])
    for i in (0, 16383, 16384):
        f, end = zstd_format.decode_frame(whole[offs[i]:offs[i + 1]])
        assert end == lens[i] and f["data"] == zstd_sim.rebuild(frames[i])     # (nine bytes: the block is written Raw)


# ------------------------------------------------------------------ partial delivery
HW = 16384
N = 4 * HW + 1000


@pytest.fixture(scope="module")
def five_chunks():
    return datagen.gen_bytes("silesia", N, 91)


def _hw_framing(s, on=1):
    s.L.qzamd_set_hw_framing.argtypes = [C.c_void_p, C.c_int]
    assert s.L.qzamd_set_hw_framing(C.byref(s.s), on) == A.QZ_OK


def _gzip_ext_members(full):
    """lengths of the hardware path's members: 24 bytes of header with the compressed length at 20, 8 of trailer"""
    lens, pos = [], 0
    while pos < len(full):
        assert full[pos:pos + 4] == b"\x1f\x8b\x08\x04" and full[pos + 12:pos + 14] == b"QZ"
        lens.append(24 + int.from_bytes(full[pos + 20:pos + 24], "little") + 8)
        pos += lens[-1]
    assert pos == len(full)
    return lens


def _device_lens(fn, src, chunk, bound, **kw):
    c = qatzip_amd.Context(0)
    try:
        d_src = c.alloc(len(src)); d_src.upload(src)
        d_dst = c.alloc(bound + 64)
        n, lens = getattr(c, fn)(d_src, len(src), d_dst, chunk, **kw)
        out = d_dst.download(n).tobytes()
        d_src.free(); d_dst.free()
    finally:
        c.close()
    return out, [int(x) for x in lens]


def _session_and_items(path, src):
    """-> (session, the output of a call with ample room, its item lengths); the lengths from outside the session"""
    if path == "deflate_hw":
        s = A.Session(A.QZ_DEFLATE_GZIP_EXT, HW); _hw_framing(s)
        full = s.compress(src, 1)[2]
        return s, full, _gzip_ext_members(full)
    if path == "lz4_hw":
        s = A.Session(lz4=True, hw_buff_sz=HW); _hw_framing(s)
        dev, lens = _device_lens("lz4_compress_frames", src, HW, len(src) + 5 * 64, hw=True)
    elif path == "lz4s":
        s = A.Session(lz4s=True, hw_buff_sz=HW)
        dev, lens = _device_lens("lz4s_compress_blocks", src, HW, lz4s_bound(len(src), HW))
    else:
        s = A.Session(zstd=True, hw_buff_sz=HW)
        dev, lens = _device_lens("zstd_compress_frames", src, HW, zstd_bound(len(src), HW))
    assert s.rc_setup == A.QZ_OK
    full = s.compress(src, 1)[2]
    assert full == dev
    return s, full, lens


@pytest.mark.parametrize("path", ["deflate_hw", "lz4_hw", "lz4s", "zstd"])
def test_whole_items_that_fit(path, five_chunks):
    src = five_chunks
    s, full, lens = _session_and_items(path, src)
    assert len(lens) == 5 and sum(lens) == len(full)
    rc, used, out, _ = s.compress(src, 1, cap=len(full))
    assert (rc, used) == (A.QZ_OK, N) and out == full
    three = lens[0] + lens[1] + lens[2]
    tin, tout = s.s.total_in, s.s.total_out
    for cap, items in ((three, 3), (three - 1, 2), (lens[0] - 1, 0)):
        rc, used, out, _ = s.compress(src, 1, cap=cap)
        assert (rc, used) == (A.QZ_BUF_ERROR, items * HW), (path, cap)
        assert out == full[:sum(lens[:items])], (path, cap)
        tin += items * HW; tout += len(out)
        assert (s.s.total_in, s.s.total_out) == (tin, tout), (path, cap)
    s.close()


def test_software_framing_keeps_the_trailer_with_the_last_chunk(five_chunks):
    """one gzip member per call behind a ten-byte header: chunks that fit behind the header, and the trailer only together
    with the last chunk - when everything but the trailer fits, the last chunk waits for the next call (src/qatzip_sw.c:
    the trailer is written by the call that consumes the stream's end)"""
    src = five_chunks
    s = A.Session(A.QZ_DEFLATE_GZIP, HW)
    rc, used, full, _ = s.compress(src, 1)
    assert (rc, used) == (A.QZ_OK, N)
    # the first k chunks of a stream that stays open are the first k chunks of the closed one: each ends on a flush marker
    ends = []
    for k in (1, 2, 3, 4):
        o = A.Session(A.QZ_DEFLATE_GZIP, HW)
        rc, used, out, _ = o.compress(src[:k * HW], 0)
        assert (rc, used) == (A.QZ_OK, k * HW) and out == full[:len(out)]
        ends.append(len(out))
        o.close()
    assert 10 < ends[0] < ends[1] < ends[2] < ends[3] < len(full) - 8
    for cap, items in ((ends[2], 3), (ends[2] - 1, 2), (ends[0] - 1, 0),
                       (len(full) - 1, 4), (len(full) - 8, 4), (ends[3], 4)):     # the trailer is what does not fit
        rc, used, out, _ = s.compress(src, 1, cap=cap)
        assert (rc, used) == (A.QZ_BUF_ERROR, items * HW), cap
        assert out == (full[:ends[items - 1]] if items else b""), cap
        if items:                                                   # the stream is open now: the rest closes it
            rc, used, rest, _ = s.compress(src[items * HW:], 1)
            assert (rc, used) == (A.QZ_OK, N - items * HW) and out + rest == full
    rc, used, out, _ = s.compress(src, 1, cap=len(full))
    assert (rc, used) == (A.QZ_OK, N) and out == full
    s.close()
