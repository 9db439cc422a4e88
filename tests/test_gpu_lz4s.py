"""LZ4s on the GPU: the device layer (qzd_lz4s_compress_blocks) gives the streams the CPU emulator pinned in
tests/golden/lz4s/index.json (made by tests/golden/gen_lz4s.py) - the two builds of qzk_lz4s.h write the same bytes - and
every stream is read back by the independent reader tests/lz4s_format.py; LZ4s sessions through include/qatzip.h: blocks
that fit, the post-processing callback's contract, what the sessions still refuse, and two threads at once."""
import ctypes as C
import hashlib
import json
import os
import threading

import pytest

import lz4s_format as F
import lz4s_sim
import qatzip_amd
from qatzip_amd import api as A
from qatzip_amd._lib import lz4s_bound

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "lz4s", "index.json")) as f:
    INDEX = json.load(f)

HW = 65536


def _sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def ctx():
    c = qatzip_amd.Context(0)
    yield c
    c.close()


def device_blocks(ctx, src, hw=HW, mm=3, level=1):
    d_src = ctx.alloc(max(len(src), 1)); d_src.upload(src)
    d_dst = ctx.alloc(lz4s_bound(len(src), hw) + 64)
    n, lens = ctx.lz4s_compress_blocks(d_src, len(src), d_dst, hw, mm, level, dst_cap=lz4s_bound(len(src), hw))
    out = d_dst.download(n).tobytes()
    d_src.free(); d_dst.free()
    assert int(lens.sum()) == n
    return out, lens


@pytest.fixture(scope="module")
def five(ctx):
    """five chunks of 64 KB (the last one short) and their blocks from the device layer, shared by the session tests"""
    src = lz4s_sim.make_input("silesia", 4 * HW + 12345, 21)
    out, lens = device_blocks(ctx, src)
    assert F.decode(out, 3, HW) == src and len(lens) == 5
    return src, out, [int(x) for x in lens]


def test_every_pinned_case_equals_the_emulator(ctx):
    assert len(INDEX["cases"]) >= 20
    for c in INDEX["cases"]:
        src = lz4s_sim.make_input(c["kind"], c["n"], c["seed"])
        assert _sha(src) == c["in_sha"], c
        out, _ = device_blocks(ctx, src, c["hw_buff_sz"], c["mini_match"])
        assert (len(out), _sha(out)) == (c["out_len"], c["out_sha"]), c
        assert F.decode(out, c["mini_match"], c["hw_buff_sz"]) == src


def test_every_level_runs_the_same_parse_and_bad_arguments_are_refused(ctx, five):
    src, out, _ = five
    for lvl in (2, 12):
        assert device_blocks(ctx, src, level=lvl)[0] == out
    d = ctx.alloc(4096); big = ctx.alloc(lz4s_bound(1000, 1024) + 64)
    ol = C.c_uint64(0)
    call = ctx.L.qzd_lz4s_compress_blocks
    assert call(ctx.h, d.ptr, 1000, 1024, 3, 1, big.ptr, lz4s_bound(1000, 1024) - 1, C.byref(ol), None) == -3     # QZD_ERR_DSTCAP
    assert call(ctx.h, d.ptr, 1000, 1024, 3, 0, big.ptr, big.nbytes, C.byref(ol), None) == -5                     # QZD_ERR_UNSUPPORTED
    assert call(ctx.h, d.ptr, 1000, 1024, 3, 13, big.ptr, big.nbytes, C.byref(ol), None) == -5
    for hw, mm in ((512, 3), (1025, 3), (1 << 20, 3), (1024, 2), (1024, 5)):
        assert call(ctx.h, d.ptr, 1000, hw, mm, 1, big.ptr, big.nbytes, C.byref(ol), None) == -1                  # QZD_ERR_PARAM
    assert call(ctx.h, d.ptr, 1000, 1024, 3, 1, None, big.nbytes, C.byref(ol), None) == -1
    assert call(ctx.h, d.ptr, 1000, 1024, 3, 1, big.ptr, big.nbytes, None, None) == -1
    ol.value = 7
    assert call(ctx.h, d.ptr, 0, 1024, 3, 1, big.ptr, big.nbytes, C.byref(ol), None) == 0 and ol.value == 0       # n == 0 writes nothing
    d.free(); big.free()


def test_many_chunks_by_persistent_waves(ctx):
    """4 MiB at 64 KB chunks and at 1 KB chunks (4096 blocks: more than the device holds waves), checked by decoding"""
    src = lz4s_sim.make_input("silesia", 4 << 20, 33)
    for hw, mm in ((HW, 3), (1024, 4)):
        out, lens = device_blocks(ctx, src, hw, mm)
        assert len(lens) == (4 << 20) // hw
        assert F.decode(out, mm, hw) == src


def test_qzcompress_without_callback(five):
    src, blocks, lens = five
    s = A.Session(lz4s=True)
    assert s.rc_setup == A.QZ_OK
    rc, used, out, _ = s.compress(src, 1)
    assert (rc, used) == (A.QZ_OK, len(src)) and out == blocks
    assert (s.s.total_in, s.s.total_out) == (len(src), len(blocks))
    # last is validated and otherwise ignored
    rc, used, out, _ = s.compress(src, 0)
    assert (rc, used) == (A.QZ_OK, len(src)) and out == blocks
    assert s.compress(src, 2)[0] == A.QZ_PARAMS
    assert (s.s.total_in, s.s.total_out) == (2 * len(src), 2 * len(blocks))
    # a destination that holds exactly two of the five blocks
    rc, used, out, _ = s.compress(src, 1, cap=lens[0] + lens[1])
    assert (rc, used) == (A.QZ_BUF_ERROR, 2 * HW) and out == blocks[:lens[0] + lens[1]]
    assert F.decode(out, 3, HW) == src[:2 * HW]
    rc, used, out, _ = s.compress(src, 1, cap=lens[0] + lens[1] + lens[2] - 1)
    assert (rc, used, len(out)) == (A.QZ_BUF_ERROR, 2 * HW, lens[0] + lens[1])
    # not even one block
    rc, used, out, _ = s.compress(src, 1, cap=3)
    assert (rc, used, out) == (A.QZ_BUF_ERROR, 0, b"")
    # small calls go to the GPU too; the CRC is that of the input consumed, chained
    rc, used, out, crc = s.compress(src[:1], 1, crc0=0)
    assert (rc, used) == (A.QZ_OK, 1) and out == b"\x02\x00\x00\x00\x10" + src[:1]
    import zlib
    rc, used, out, crc = s.compress(src[:HW + 5], 1, crc0=0)
    assert rc == A.QZ_OK and crc == zlib.crc32(src[:HW + 5])
    rc, used, out, crc = s.compress(src[HW + 5:], 1, crc0=crc)
    assert rc == A.QZ_OK and crc == zlib.crc32(src)
    rc, used, out, crc = s.compress(src, 1, cap=lens[0], crc0=0)
    assert (rc, used) == (A.QZ_BUF_ERROR, HW) and crc == zlib.crc32(src[:HW])
    # what an LZ4s session still refuses
    rc, used, back = s.decompress(blocks, len(src))
    assert rc == A.QZ_UNSUPPORTED_FMT
    strm = A.QzStream()
    buf_in, buf_out = C.create_string_buffer(src[:100], 100), C.create_string_buffer(1000)
    strm.in_ = C.cast(buf_in, C.c_void_p); strm.out = C.cast(buf_out, C.c_void_p); strm.in_sz = 100; strm.out_sz = 1000
    assert s.L.qzCompressStream(C.byref(s.s), C.byref(strm), 1) == A.QZ_PARAMS
    assert s.L.qzDecompressStream(C.byref(s.s), C.byref(strm), 1) == A.QZ_PARAMS
    s.close()


def test_mini_match_4_and_larger_chunks_through_the_session(ctx):
    src = lz4s_sim.make_input("text", 300000, 8)
    s = A.Session(lz4s=True, mini_match=4, hw_buff_sz=131072, comp_lvl=9)
    assert s.rc_setup == A.QZ_OK
    rc, used, out, _ = s.compress(src, 1)
    assert (rc, used) == (A.QZ_OK, len(src)) and out == device_blocks(ctx, src, 131072, 4)[0]
    data, st = F.decode_stats(out, 4, 131072)
    assert data == src and min(x["shortest_match"] for x in st) >= 4
    s.close()


def test_callback_that_succeeds(five):
    src, blocks, lens = five
    seen = {}

    def cb(ext, p_src, p_src_len, p_dest, p_dest_len, p_status):
        seen["ext"], seen["src"], seen["src_len"], seen["dest_len"] = ext, p_src, p_src_len[0], p_dest_len[0]
        seen["lz4s"] = C.string_at(p_dest, p_dest_len[0])          # copied before it is overwritten
        C.memmove(p_dest, b"0123456789", 10)
        p_dest_len[0] = 10
        return A.QZ_OK
    s = A.Session(lz4s=True, callback=cb, external=0xABCD)
    assert s.rc_setup == A.QZ_OK
    buf = C.create_string_buffer(src, len(src))
    rc, used, out, ext_rc = s.compress_ext(buf, 1)
    assert (rc, used, out, ext_rc) == (A.QZ_OK, len(src), b"0123456789", 0)
    assert seen["src"] == C.addressof(buf) and seen["ext"] == 0xABCD
    assert seen["src_len"] == len(src) and seen["dest_len"] == len(blocks) and seen["lz4s"] == blocks
    assert (s.s.total_in, s.s.total_out) == (len(src), len(blocks))         # LZ4s bytes, before post-processing
    # QZ_BUF_ERROR with progress: the callback sees the blocks that fit
    rc, used, out, ext_rc = s.compress_ext(buf, 1, cap=lens[0] + lens[1])
    assert (rc, used, out, ext_rc) == (A.QZ_BUF_ERROR, 2 * HW, b"0123456789", 0)
    assert seen["src_len"] == 2 * HW and seen["lz4s"] == blocks[:lens[0] + lens[1]]
    s.close()


def test_callback_that_fails(five):
    src, blocks, lens = five

    def cb(ext, p_src, p_src_len, p_dest, p_dest_len, p_status):
        p_status[0] = -77
        return A.QZ_POST_PROCESS_ERROR
    s = A.Session(lz4s=True, callback=cb)
    rc, used, out, ext_rc = s.compress_ext(src, 1)
    assert rc == -117 and ext_rc == (-77) & 0xFFFFFFFFFFFFFFFF and (used, out) == (0, b"")
    assert s.s.thd_sess_stat == -117
    s.close()


def test_callback_is_not_called_without_input_or_without_a_block(five):
    src, _, _ = five
    calls = []

    def cb(ext, p_src, p_src_len, p_dest, p_dest_len, p_status):
        calls.append(p_src_len[0])
        return A.QZ_OK
    s = A.Session(lz4s=True, callback=cb)
    rc, used, out, ext_rc = s.compress_ext(b"", 1, cap=100)
    assert (rc, used, out) == (A.QZ_OK, 0, b"") and not calls
    rc, used, out, ext_rc = s.compress_ext(src, 1, cap=3)                   # QZ_BUF_ERROR with *src_len == 0
    assert (rc, used, out) == (A.QZ_BUF_ERROR, 0, b"") and not calls
    rc, used, out, ext_rc = s.compress_ext(src[:10], 1)
    assert rc == A.QZ_OK and calls == [10]
    s.close()


def test_sessionless_compress_after_set_defaults(five):
    """after qzSetDefaultsLZ4S a qzCompress on a session that was never set up makes an LZ4s session (src/qatzip.c:1902-1903).
    In a child process: the defaults are the process's."""
    import subprocess
    import sys
    src, blocks, _ = five
    child = r"""
import ctypes as C, sys, hashlib
sys.path.insert(0, %r)
import lz4s_sim
from qatzip_amd import api as A
L = A.lib()
p = A.QzSessionParamsLZ4S(); L.qzGetDefaultsLZ4S(C.byref(p))
p.common_params.direction = A.QZ_DIR_COMPRESS
assert L.qzSetDefaultsLZ4S(C.byref(p)) == A.QZ_OK
src = lz4s_sim.make_input("silesia", 4 * 65536 + 12345, 21)
s = A.QzSession()
sl, dl = C.c_uint(len(src)), C.c_uint(2 * len(src))
dst = C.create_string_buffer(2 * len(src))
assert L.qzCompress(C.byref(s), src, C.byref(sl), dst, C.byref(dl), 1) == A.QZ_OK
print(hashlib.sha256(dst.raw[:dl.value]).hexdigest())
L.qzTeardownSession(C.byref(s))
""" % HERE
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", child], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == _sha(blocks), r.stdout + r.stderr


def test_two_threads_with_a_session_each(ctx):
    calls = [lz4s_sim.make_input(("text", "records", "silesia", "lzmix")[i % 4], HW, 100 + i) for i in range(32)]
    d_src = ctx.alloc(32 * HW); d_src.upload(b"".join(calls))
    d_dst = ctx.alloc(lz4s_bound(32 * HW, HW))
    n, lens = ctx.lz4s_compress_blocks(d_src, 32 * HW, d_dst, HW, 3, 1)
    whole = d_dst.download(n).tobytes()
    d_src.free(); d_dst.free()
    expect, pos = [], 0
    for ln in lens:
        expect.append(whole[pos:pos + int(ln)]); pos += int(ln)
    got = [[None] * 32, [None] * 32]

    def work(t):
        s = A.Session(lz4s=True)
        for i, c in enumerate(calls):
            got[t][i] = s.compress(c, 1)
        s.close()
    th = [threading.Thread(target=work, args=(t,)) for t in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for t in (0, 1):
        for i in range(32):
            rc, used, out, _ = got[t][i]
            assert (rc, used) == (A.QZ_OK, HW) and out == expect[i], (t, i)
