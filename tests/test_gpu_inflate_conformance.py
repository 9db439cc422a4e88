"""The inflate kernels on the GPU against zlib, on hand-built deflate edge cases (tests/deflate_writer.py), and the
hand-back branch of the K-lanes-per-segment phase A (qzd_inflate.hip, two_phase()) with its decode counters.

Every case goes through Context.inflate_stream with the wave-per-segment kernel and the two-phase kernels (serial phase A
and K = 4 / 8 / 16 / 32), with the exact segment size as the hint and with none; alone, and as a member of eight segments
with the case in each one at another bit phase.  The invalid cases are checked on the emulator first
(test_sim_inflate_conformance.py); here each must end in QzdError with nothing written past the destination."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import deflate_writer as W

pytestmark = pytest.mark.gpu

CONFIGS = [("wave", None), ("lane", None), ("lane", "4"), ("lane", "8"), ("lane", "16"), ("lane", "32")]
CANARY = 4096


@pytest.fixture(scope="module")
def ctx():
    import qatzip_amd
    c = qatzip_amd.Context(0)
    yield c
    c.close()


def _config(monkeypatch, mode, k):
    monkeypatch.setenv("QATZIP_AMD_INFLATE", mode)
    if k:
        monkeypatch.setenv("QATZIP_AMD_INFLATE_K", k)
    else:
        monkeypatch.delenv("QATZIP_AMD_INFLATE_K", raising=False)


def _inflate(ctx, comp, cap, hint):
    """qzd_inflate_stream with a destination of exactly cap bytes, followed by CANARY bytes of 0xAA that must stay as they
    are.  -> (in_used, bytes, crc) or the QzdError"""
    import qatzip_amd
    d_src = ctx.alloc(len(comp)); d_src.upload(comp)
    d_dst = ctx.alloc(cap + CANARY); d_dst.upload(np.full(cap + CANARY, 0xAA, np.uint8))
    iu, ol, crc = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    try:
        try:
            ctx._chk(ctx.L.qzd_inflate_stream(ctx.h, d_src.ptr, len(comp), d_dst.ptr, cap, hint, C.byref(iu), C.byref(ol),
                                              C.byref(crc)))
            got = d_dst.download(cap + CANARY).tobytes()
            result = (iu.value, got[:ol.value], crc.value)
        except qatzip_amd.QzdError as e:
            got = d_dst.download(cap + CANARY).tobytes()
            result = e
        assert got[cap:] == b"\xaa" * CANARY, "written past the destination's end"
    finally:
        d_src.free(); d_dst.free()
    return result


def _lone_and_members(name, fn):
    comp = W.build_case(fn)
    ok, want, in_used = W.reference(comp)
    assert ok, name
    yield "alone", comp, want, in_used, max(len(want), 1)
    member, seg_out = W.build_member(fn, len(want))
    ok, want, in_used = W.reference(member)
    assert ok, name
    yield "member", member, want, in_used, seg_out


@pytest.mark.parametrize("mode,k", CONFIGS)
def test_valid_corpus_decodes_to_zlibs_bytes(ctx, monkeypatch, mode, k):
    _config(monkeypatch, mode, k)
    for name, fn in sorted(W.VALID.items()):
        for where, comp, want, in_used, seg in _lone_and_members(name, fn):
            for hint in (seg, 0):
                r = _inflate(ctx, comp, len(want), hint)
                assert not isinstance(r, Exception), (name, where, hint, mode, k, str(r))
                iu, got, crc = r
                assert got == want, (name, where, hint, mode, k)
                assert iu == in_used and crc == zlib.crc32(want) & 0xffffffff, (name, where, hint, mode, k, iu, in_used)


@pytest.mark.parametrize("mode,k", CONFIGS)
def test_invalid_corpus_is_a_data_error(ctx, monkeypatch, mode, k):
    import qatzip_amd
    _config(monkeypatch, mode, k)
    for name, fn in sorted(W.INVALID.items()):
        streams = [("alone", W.build_case(fn))]
        if name not in W.LONE_ONLY:
            streams.append(("member", W.build_member(fn, 0, where={3})[0]))      # the bad segment among good ones
        for where, comp in streams:
            assert not W.reference(comp)[0], (name, where, "zlib accepts it")
            for hint in (24576, 0):
                r = _inflate(ctx, comp, 1 << 18, hint)
                assert isinstance(r, qatzip_amd.QzdError), (name, where, hint, mode, k)
                assert "rc=%d:" % -4 in str(r), (name, where, hint, mode, k, str(r))       # QZD_ERR_DATA


def _gzip(raw, data):
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data) & 0xffffffff)


def _zlib(raw, data):
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data) & 0xffffffff)


def test_valid_corpus_through_the_api():
    """each valid case as a GZIP member and as a ZLIB stream through qzDecompress: zlib.decompress is the reference"""
    import qatzip_amd.api as A
    sg, sz = A.Session(A.QZ_DEFLATE_GZIP, 65536), A.Session(hw_buff_sz=65536, zlib_format=True)
    for name, fn in sorted(W.VALID.items()):
        for comp in (W.build_case(fn), W.build_case(fn, 20480, 5)):
            ok, want, in_used = W.reference(comp)
            raw = comp[:in_used]
            for s, member, wbits in ((sg, _gzip(raw, want), 31), (sz, _zlib(raw, want), 15)):
                assert zlib.decompress(member, wbits) == want
                rc, used, back = s.decompress(member, len(want) + 64)
                assert rc == A.QZ_OK and back == want and used == len(member), (name, wbits, rc, used, len(member))
    sg.close(); sz.close()


# ---- the hand-back branch ----

SEG = 65536
NSEG = 256
R = 64                          # QZK_SPEC_HANDBACK(256): whole-segment regions of the hand-back area


@pytest.fixture(scope="module")
def handback_parts():
    """the bytes of an ordinary segment (64 KiB of text, one dynamic block) and of a hand-back segment (length-3 matches),
    each with a sync-flush marker and in a last-segment (BFINAL) version, and what they decode to"""
    data, toks = W.content_tokens(SEG, 7)
    parts = {}
    for final in (0, 1):
        w = W.BitWriter()
        W.ordinary_block(w, toks, final=final)
        if not final:
            W.sync_flush(w)
        parts[("plain", final)] = w.getvalue()
        parts[("m3", final)] = W.match3_segment(SEG, final)
    outs = {}
    for kind in ("plain", "m3"):
        ok, o, iu = W.reference(parts[(kind, 1)])
        assert ok and len(o) == SEG and iu == len(parts[(kind, 1)])
        outs[kind] = o
    return parts, outs


def _handback_member(handback_parts, nback):
    """NSEG segments, nback of them (spread evenly) made to be handed back -> (stream, output, segment records)"""
    parts, outs = handback_parts
    back = set(np.linspace(0, NSEG - 1, nback).round().astype(int).tolist()) if nback else set()
    assert len(back) == nback
    comp, out, segs = [], [], []
    off = 0
    for i in range(NSEG):
        kind = "m3" if i in back else "plain"
        p = parts[(kind, int(i == NSEG - 1))]
        segs.append((off, i * SEG, len(p), SEG, 0, len(p)))
        comp.append(p); out.append(outs[kind]); off += len(p)
    return b"".join(comp), b"".join(out), segs


def _decode_both_ways(ctx, comp, out, segs):
    """run_b = false (inflate_stream with the segment size as its hint) and run_b = true (inflate_segments with every
    segment's compressed length): bytes and CRC against the input; -> the counters of each, read and reset"""
    ctx.inflate_stats(reset=True)
    d_src = ctx.alloc(len(comp)); d_src.upload(comp)
    d_dst = ctx.alloc(len(out))
    try:
        iu, ol, crc = ctx.inflate_stream(d_src, len(comp), d_dst, SEG)
        assert iu == len(comp) and ol == len(out) and crc == zlib.crc32(out) & 0xffffffff
        assert d_dst.download(ol).tobytes() == out
        stream_stats = ctx.inflate_stats(reset=True)
        d_dst.upload(np.zeros(len(out), np.uint8))
        res = ctx.inflate_segments(d_src, d_dst, segs)
        assert (res["status"] >= 0).all() and [int(x) for x in res["out_len"]] == [SEG] * NSEG
        assert [int(x) for x in res["in_used"]] == [s[2] for s in segs]
        assert ctx.crc32(d_dst, len(out)) == zlib.crc32(out) & 0xffffffff
        assert d_dst.download(len(out)).tobytes() == out
        seg_stats = ctx.inflate_stats(reset=True)
    finally:
        d_src.free(); d_dst.free()
    return stream_stats, seg_stats


def test_ordinary_segments_hand_nothing_back(ctx, monkeypatch, handback_parts):
    monkeypatch.delenv("QATZIP_AMD_INFLATE", raising=False)
    monkeypatch.delenv("QATZIP_AMD_INFLATE_K", raising=False)
    comp, out, segs = _handback_member(handback_parts, 0)
    assert _decode_both_ways(ctx, comp, out, segs) == ((0, 0), (0, 0))


@pytest.mark.parametrize("nback,reruns", [(R, 0), (R + 1, 1), (NSEG, 1)])
def test_handed_back_segments(ctx, monkeypatch, handback_parts, nback, reruns):
    """(a) exactly R hand-backs fill the hand-back area, (b) R + 1 re-run the call with one lane a segment, (c) every
    segment handed back - through run_b = false and run_b = true alike"""
    monkeypatch.delenv("QATZIP_AMD_INFLATE", raising=False)
    monkeypatch.delenv("QATZIP_AMD_INFLATE_K", raising=False)
    comp, out, segs = _handback_member(handback_parts, nback)
    assert _decode_both_ways(ctx, comp, out, segs) == ((nback, reruns), (nback, reruns))


def test_all_segments_handed_back_through_the_api_and_three_waves(ctx, monkeypatch, handback_parts):
    """case (c) once more as one GZIP file through qzDecompress, and through inflate_stream with three waves a SIMD"""
    import qatzip_amd.api as A
    monkeypatch.delenv("QATZIP_AMD_INFLATE", raising=False)
    monkeypatch.delenv("QATZIP_AMD_INFLATE_K", raising=False)
    comp, out, segs = _handback_member(handback_parts, NSEG)
    member = _gzip(comp, out)
    assert gzip.decompress(member) == out
    s = A.Session(A.QZ_DEFLATE_GZIP, 65536)
    rc, used, back = s.decompress(member, len(out) + 64)
    s.close()
    assert rc == A.QZ_OK and used == len(member) and back == out
    monkeypatch.setenv("QATZIP_AMD_INFLATE_OCC", "3")
    assert _decode_both_ways(ctx, comp, out, segs) == ((NSEG, 1), (NSEG, 1))
