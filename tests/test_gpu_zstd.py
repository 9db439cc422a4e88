"""Zstd sessions on the GPU: the device layer (qzd_zstd_compress_frames) gives the streams the CPU emulator pinned in
tests/golden/zstd/index.json (made by tests/golden/gen_zstd.py, where every stream was also decoded by libzstd) - the two
builds of qzk_zstd.h write the same bytes; the entropy stage alone (qzd_zstd_encode_frames) at the format's switches; zstd
sessions through include/qzamd_zstd.h.  Every frame is read by the strict reader tests/zstd_format.py; libzstd is used where
it loads and required nowhere."""
import ctypes as C
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import lz4s_sim
import zstd_format as Z
import zstd_ref
import zstd_sim as S
import qatzip_amd
from qatzip_amd import api as A
from qatzip_amd._lib import lz4s_bound, zstd_bound

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HW = 16384


def _sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def ctx():
    c = qatzip_amd.Context(0)
    yield c
    c.close()


def device_frames(ctx, src, hw=HW, mm=3, level=1):
    d_src = ctx.alloc(max(len(src), 1)); d_src.upload(src)
    d_dst = ctx.alloc(zstd_bound(len(src), hw) + 64)
    n, lens = ctx.zstd_compress_frames(d_src, len(src), d_dst, hw, mm, level, dst_cap=zstd_bound(len(src), hw))
    out = d_dst.download(n).tobytes()
    d_src.free(); d_dst.free()
    assert int(lens.sum()) == n
    return out, [int(x) for x in lens]


def device_encode(ctx, frames):
    lits, seqs, desc = S.pack_frames(frames)
    d_l = ctx.alloc(len(lits) + 16); d_l.upload(lits + b"\0")
    d_s = ctx.alloc(seqs.nbytes + 16); d_s.upload(np.concatenate([seqs, np.zeros(3, np.uint32)]).tobytes())
    cap = sum(min(f[0], Z.MAX_BLOCK) + 12 for f in frames)
    d_dst = ctx.alloc(cap + 64)
    rc, n, lens = ctx.zstd_encode_frames(d_l, d_s, desc, d_dst, dst_cap=cap)
    out = d_dst.download(n).tobytes() if n else b""
    d_l.free(); d_s.free(); d_dst.free()
    return rc, out, [int(x) for x in lens]


@pytest.fixture(scope="module")
def five(ctx):
    """five chunks of 16 KB (the last one short) and their frames from the device layer, shared by the session tests"""
    src = S.make_input("silesia", 4 * HW + 1234, 21)
    out, lens = device_frames(ctx, src)
    assert Z.decode(out, HW) == src and len(lens) == 5
    zstd_ref.check(out, src)
    return src, out, lens


def test_every_pinned_case_equals_the_emulator(ctx):
    cases = S.index()["cases"]
    assert len(cases) >= 20
    for c in cases:
        src = S.make_input(c["kind"], c["n"], c["seed"])
        assert _sha(src) == c["in_sha"], c
        out, _ = device_frames(ctx, src, c["hw_buff_sz"], c["mini_match"])
        assert (len(out), _sha(out)) == (c["out_len"], c["out_sha"]), c


def test_device_layer_arguments(ctx, five):
    src, out, _ = five
    assert device_frames(ctx, src, level=12)[0] == out
    d = ctx.alloc(4096); big = ctx.alloc(zstd_bound(1000, 1024) + 64)
    ol = C.c_uint64(0)
    call = ctx.L.qzd_zstd_compress_frames
    assert zstd_bound(1000, 1024) == 1012 and zstd_bound(3000, 1024) == 3000 + 36
    assert call(ctx.h, d.ptr, 1000, 1024, 3, 1, big.ptr, 1011, C.byref(ol), None) == -3                           # QZD_ERR_DSTCAP
    assert call(ctx.h, d.ptr, 1000, 1024, 3, 0, big.ptr, big.nbytes, C.byref(ol), None) == -5                     # QZD_ERR_UNSUPPORTED
    for hw, mm in ((512, 3), (1025, 3), (262144, 3), (1024, 2), (1024, 5)):
        assert call(ctx.h, d.ptr, 1000, hw, mm, 1, big.ptr, big.nbytes, C.byref(ol), None) == -1                  # QZD_ERR_PARAM
    assert call(ctx.h, d.ptr, 1000, 1024, 3, 1, None, big.nbytes, C.byref(ol), None) == -1
    ol.value = 7
    assert call(ctx.h, d.ptr, 0, 1024, 3, 1, big.ptr, big.nbytes, C.byref(ol), None) == 0 and ol.value == 0       # n == 0 writes nothing
    d.free(); big.free()


def test_more_chunks_than_waves(ctx):
    """256 KB at 1 KB chunks, checked by decoding"""
    src = S.make_input("silesia", 262144, 33)
    out, lens = device_frames(ctx, src, 1024, 4)
    assert len(lens) == 256 and Z.decode(out, 1024) == src
    zstd_ref.check(out, src)


def test_encode_frames_at_the_switches(ctx):
    names = ("count127", "count128", "count7eff", "count7f00", "huf1023", "huf1024", "top128", "top129", "rle", "ll65536")
    rc, out, lens = device_encode(ctx, [S.EDGES[k] for k in names])
    assert rc == 0 and sum(lens) == len(out)
    pos = 0
    got = {}
    for k, ln in zip(names, lens):
        f, end = Z.decode_frame(out[pos:pos + ln])
        assert end == ln and f["data"] == S.rebuild(S.EDGES[k]) and f["sequences"] == S.EDGES[k][1], k
        zstd_ref.check(out[pos:pos + ln], f["data"])
        got[k] = f
        pos += ln
    assert [got[k]["seq"]["count"] for k in names[:4]] == [127, 128, 0x7eff, 0x7f00]
    assert got["huf1023"]["literals"]["streams"] == 1 and got["huf1024"]["literals"]["streams"] == 4
    assert got["top128"]["literals"]["description"] == "direct" and got["top129"]["literals"]["description"] == "fse"
    # the emulator writes the same bytes
    rc, sim, _ = S.encode([S.EDGES[k] for k in names])
    assert rc == 0 and sim == out


def test_encode_frames_refusals(ctx):
    for name in ("sum_short", "offset0", "offset_beyond", "match2"):
        rc, out, _ = device_encode(ctx, [S.EDGES["rle"], S.REFUSED[name][0]])
        assert rc == -4 and out == b"", name                                                                       # QZD_ERR_DATA
    for name in ("content_above_128k", "content0", "literals_above_content", "records_above_a_third"):
        rc, out, _ = device_encode(ctx, [S.REFUSED[name][0]])
        assert rc == -1 and out == b"", name                                                                       # QZD_ERR_PARAM


def test_session_five_chunks(five):
    src, frames, lens = five
    s = A.Session(zstd=True, hw_buff_sz=HW)
    assert s.rc_setup == A.QZ_OK
    assert s.L.qzMaxCompressedLength(len(src), C.byref(s.s)) == Z.bound(len(src), HW) == len(src) + 5 * 12
    rc, used, out, _ = s.compress(src, 1)
    assert (rc, used) == (A.QZ_OK, len(src)) and out == frames
    assert (s.s.total_in, s.s.total_out) == (len(src), len(frames))
    assert s.compress(src, 2)[0] == A.QZ_PARAMS
    # a destination that holds exactly two of the five frames, then one byte less than three
    rc, used, out, _ = s.compress(src, 1, cap=lens[0] + lens[1])
    assert (rc, used) == (A.QZ_BUF_ERROR, 2 * HW) and out == frames[:lens[0] + lens[1]]
    assert Z.decode(out, HW) == src[:2 * HW]
    rc, used, out, _ = s.compress(src, 1, cap=lens[0] + lens[1] + lens[2] - 1)
    assert (rc, used, len(out)) == (A.QZ_BUF_ERROR, 2 * HW, lens[0] + lens[1])
    assert (s.s.total_in, s.s.total_out) == (len(src) + 4 * HW, len(frames) + 2 * (lens[0] + lens[1]))
    # not even one frame
    rc, used, out, _ = s.compress(src, 1, cap=3)
    assert (rc, used, out) == (A.QZ_BUF_ERROR, 0, b"")
    # an empty call, and a small one: on the GPU too
    rc, used, out, _ = s.compress(b"", 1, cap=100)
    assert (rc, used, out) == (A.QZ_OK, 0, b"")
    rc, used, out, _ = s.compress(src[:1], 1)
    assert (rc, used) == (A.QZ_OK, 1) and out == Z.MAGIC + b"\x20\x01" + b"\x09\x00\x00" + src[:1]
    # crc: that of the input consumed, chained
    rc, used, out, crc = s.compress(src[:HW + 5], 1, crc0=0)
    assert rc == A.QZ_OK and crc == zlib.crc32(src[:HW + 5])
    rc, used, out, crc = s.compress(src[HW + 5:], 1, crc0=crc)
    assert rc == A.QZ_OK and crc == zlib.crc32(src)
    rc, used, out, crc = s.compress(src, 1, cap=lens[0], crc0=0)
    assert (rc, used) == (A.QZ_BUF_ERROR, HW) and crc == zlib.crc32(src[:HW])
    rc, used, out, ext_rc = s.compress_ext(src, 1)
    assert (rc, used) == (A.QZ_OK, len(src)) and out == frames
    s.close()


def test_session_mini_match_4_at_128k(ctx):
    src = S.make_input("text", 300000, 8)
    s = A.Session(zstd=True, mini_match=4, hw_buff_sz=131072, comp_lvl=9)
    assert s.rc_setup == A.QZ_OK
    rc, used, out, _ = s.compress(src, 1)
    assert (rc, used) == (A.QZ_OK, len(src)) and out == device_frames(ctx, src, 131072, 4)[0]
    frames = Z.decode_frames(out)
    assert b"".join(f["data"] for f in frames) == src
    assert min(ml for f in frames for _, ml, _ in f["sequences"]) >= 4
    assert frames[0]["sequences"] == S.expected_sequences(src[:131072], 131072, 4)[0]
    s.close()


def test_setup_refusals():
    for kw in (dict(hw_buff_sz=262144), dict(hw_buff_sz=1025), dict(mini_match=5), dict(comp_lvl=13),
               dict(callback=lambda *a: 0)):
        s = A.Session(zstd=True, **kw)
        assert s.rc_setup == A.QZ_PARAMS and not s.s.internal, kw
    L = A.lib()
    p = A.QzSessionParamsLZ4S(); L.qzGetDefaultsLZ4S(C.byref(p))
    p.common_params.comp_algorithm = A.QZ_LZ4s
    for d in (A.QZ_DIR_DECOMPRESS, A.QZ_DIR_BOTH):
        p.common_params.direction = d
        q = A.QzSession()
        assert L.qzSetupSessionZstdAMD(C.byref(q), C.byref(p)) == A.QZ_PARAMS
    assert A.Session(zstd=True, hw_buff_sz=131072).rc_setup == A.QZ_OK


def _refusals(s, src, comp):
    """what a session answers to the calls an LZ4s session refuses"""
    out = [s.decompress(comp, len(src))[0]]
    strm = A.QzStream()
    buf_in, buf_out = C.create_string_buffer(src[:100], 100), C.create_string_buffer(1000)
    strm.in_ = C.cast(buf_in, C.c_void_p); strm.out = C.cast(buf_out, C.c_void_p); strm.in_sz = 100; strm.out_sz = 1000
    out.append(s.L.qzCompressStream(C.byref(s.s), C.byref(strm), 1))
    out.append(s.L.qzDecompressStream(C.byref(s.s), C.byref(strm), 1))
    r = A.QzResult(); r.src_len = 100; r.dest_len = 1000
    out.append(s.L.qzCompress2(C.byref(s.s), buf_in, buf_out, None, C.byref(r)))
    out.append(r.status)
    out.append(s.compress_crc64(src[:100])[0])
    meta = A.Metadata(len(src), HW) if hasattr(A, "Metadata") else None
    if meta is not None:
        out.append(s.compress_meta(src, meta, 0)[0])
    return out


def test_the_refusals_of_an_lz4s_session_with_the_same_codes(five):
    src, frames, _ = five
    z = A.Session(zstd=True, hw_buff_sz=HW)
    l4 = A.Session(lz4s=True, hw_buff_sz=HW)
    assert z.rc_setup == A.QZ_OK and l4.rc_setup == A.QZ_OK
    a, b = _refusals(z, src, frames), _refusals(l4, src, frames)
    assert a == b and all(x != A.QZ_OK for x in a), (a, b)
    assert a[0] == A.QZ_UNSUPPORTED_FMT and a[1] == A.QZ_PARAMS and a[2] == A.QZ_PARAMS
    z.close(); l4.close()


def test_an_lz4s_session_in_the_same_process_keeps_its_pinned_bytes(ctx):
    with open(os.path.join(HERE, "golden", "lz4s", "index.json")) as f:
        idx = json.load(f)
    c = next(x for x in idx["cases"] if x["kind"] == "silesia" and x["hw_buff_sz"] == 4096)
    src = lz4s_sim.make_input(c["kind"], c["n"], c["seed"])
    z = A.Session(zstd=True, hw_buff_sz=4096, mini_match=c["mini_match"])
    l4 = A.Session(lz4s=True, hw_buff_sz=4096, mini_match=c["mini_match"])
    rc, used, zout, _ = z.compress(src, 1)
    assert rc == A.QZ_OK and Z.decode(zout, 4096) == src
    rc, used, out, _ = l4.compress(src, 1)
    assert (rc, used) == (A.QZ_OK, len(src)) and (len(out), _sha(out)) == (c["out_len"], c["out_sha"])
    assert l4.L.qzMaxCompressedLength(len(src), C.byref(l4.s)) == lz4s_bound(len(src), 4096)
    z.close(); l4.close()
