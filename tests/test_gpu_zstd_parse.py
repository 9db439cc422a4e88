"""Zstd sessions with qzSetSessionZstdParseAMD (include/qzamd_zstd_parse.h) on the GPU: sessions and the device layer's call
with a parse depth give the bytes the CPU emulator pinned in tests/golden/zstd_parse/index.json (made by
tests/golden/gen_zstd_parse.py, where every stream was also decoded by libzstd); two sessions side by side, a call of two
scratch rounds, delivery, qzstd-amd --parse-depth, and this library's own zstd decoder on the new frames.  Frames are read
by the strict reader of whole frames, tests/zstd_full_format.py."""
import ctypes as C
import hashlib
import subprocess

import pytest

import zstd_full_format as F
import zstd_parse_sim as P
import zstd_ref
import zstd_seq_sim as Q
import zstd_sim as S
import qatzip_amd
import qatzip_amd.build as B
from qatzip_amd import api as A
from qatzip_amd._lib import zstd_bound

pytestmark = pytest.mark.gpu

EDGES = P.edge_cases()


def _sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def ctx():
    c = qatzip_amd.Context(0)
    yield c
    c.close()


def _session(depth, flags=3, hw=65536, mm=3, both=False):
    s = A.Session(zstd=not both, zstd_dec=A.QZ_DIR_BOTH if both else None, hw_buff_sz=hw, mini_match=mm)
    assert s.rc_setup == A.QZ_OK
    if depth is not None:
        assert s.set_zstd_parse(depth) == A.QZ_OK
    if flags is not None:
        assert s.set_zstd_seq(flags) == A.QZ_OK
    return s


def device_frames(ctx, src, hw, mm, flags, depth):
    d_src = ctx.alloc(max(len(src), 1)); d_src.upload(src)
    d_dst = ctx.alloc(zstd_bound(len(src), hw) + 64)
    n, lens = ctx.zstd_compress_frames(d_src, len(src), d_dst, hw, mm, 1, dst_cap=zstd_bound(len(src), hw), seq_flags=flags, parse_depth=depth)
    out = d_dst.download(n).tobytes()
    d_src.free(); d_dst.free()
    assert int(lens.sum()) == n
    return out, [int(x) for x in lens]


def test_sessions_and_the_device_call_reproduce_the_pinned_edges(ctx):
    idx = P.index()["edges"]
    assert sorted(idx) == sorted(EDGES)
    sessions = {}
    for name, c in sorted(idx.items()):
        src, hw, mm, depth = EDGES[name]
        assert (hw, mm, depth, _sha(src)) == (c["hw_buff_sz"], c["mini_match"], c["depth"], c["in_sha"]), name
        if (hw, mm) not in sessions:
            sessions[hw, mm] = _session(depth, 3, hw, mm)
        s = sessions[hw, mm]
        assert s.set_zstd_parse(depth) == A.QZ_OK                   # a later call replaces the value
        rc, used, out, _ = s.compress(src, 1)
        assert (rc, used) == (A.QZ_OK, len(src)), name
        assert (len(out), _sha(out)) == (c["out_len"], c["out_sha"]), name
        dev, lens = device_frames(ctx, src, hw, mm, 3, depth)
        assert dev == out and [f["size"] for f in F.decode_frames(out)] == lens, name
    for s in sessions.values():
        s.close()
    src, hw, mm, depth = EDGES["far"]
    f = Q.read(device_frames(ctx, src, hw, mm, 3, depth)[0], src, hw)[0]
    assert (60000, 70000) in [(ml, off) for _, ml, off in f["sequences"]]


def test_sessions_reproduce_the_pinned_kinds(ctx):
    cases = P.index()["cases"]
    assert len(cases) == 8
    s = _session(16, 3)
    for c in cases:
        src = S.make_input(c["kind"], c["n"], c["seed"])
        assert _sha(src) == c["in_sha"], c
        rc, used, out, _ = s.compress(src, 1)
        assert (rc, used) == (A.QZ_OK, len(src)), c
        assert (len(out), _sha(out)) == (c["out_len"], c["out_sha"]), c
        dev, _ = device_frames(ctx, src, 65536, 3, 3, 16)
        assert dev == out, c
    s.close()
    c = cases[0]
    src = S.make_input(c["kind"], c["n"], c["seed"])
    P.check_sequences(src[:65536], Q.read(device_frames(ctx, src, 65536, 3, 3, 16)[0], src, 65536)[0]["sequences"], 3)


def test_depth_0_gives_the_default_bytes_and_two_sessions_keep_their_own(ctx):
    c = next(x for x in Q.index()["cases"] if x["kind"] == "silesia" and x["n"] == 70001 and x["mini_match"] == 3 and x["flags"] == 3)
    src = S.make_input(c["kind"], c["n"], c["seed"])
    p16 = next(x for x in P.index()["cases"] if x["kind"] == "silesia")
    with_depth, without = _session(16, 3), _session(None, 3)
    for _ in range(2):                                              # taking turns: each keeps its own bytes
        rc, used, a, _ = with_depth.compress(src, 1)
        rc2, used2, b, _ = without.compress(src, 1)
        assert (rc, used, rc2, used2) == (A.QZ_OK, len(src), A.QZ_OK, len(src))
        assert (len(a), _sha(a)) == (p16["out_len"], p16["out_sha"])
        assert (len(b), _sha(b)) == (c["out_len"], c["out_sha"])
    # a depth and then 0: the default bytes again; the sequence flags stay what they were
    assert with_depth.set_zstd_parse(0) == A.QZ_OK
    assert with_depth.compress(src, 1)[2] == b
    with_depth.close(); without.close()
    assert device_frames(ctx, src, 65536, 3, 3, 0)[0] == b
    # a depth above 256 on a live context: QZD_ERR_PARAM (-1) and the length word untouched; 256 is taken
    d = ctx.alloc(4096); big = ctx.alloc(zstd_bound(1000, 1024) + 64)
    d.upload(src[:1000])
    for depth, want in ((257, -1), (0xffffffff, -1), (256, 0)):
        ol = C.c_uint64(7)
        assert ctx.L.qzd_zstd_compress_frames_parse(ctx.h, d.ptr, 1000, 1024, 3, 1, big.ptr, big.nbytes, C.byref(ol), None, 3, depth) == want
        assert (ol.value == 7) == (want == -1)
    d.free(); big.free()


def test_a_call_of_two_scratch_rounds(ctx):
    """1 KB chunks, one chunk more than a round of the host plan holds: the bytes of the chunks one by one"""
    hw = 1024
    batch = P.round_chunks(hw, 1 << 20)
    assert batch == 4096
    n = (batch + 1) * hw
    src = (S.make_input("silesia", 65536, 2) * (n // 65536 + 1))[:n]
    out, lens = device_frames(ctx, src, hw, 3, 3, 4)
    assert len(lens) == batch + 1
    assert F.decode(out) == src
    # the first chunks and the one in the second round against the emulator
    want, wl = P.compress(src[:4 * hw], hw, 3, 3, 4)
    assert out[:len(want)] == want and lens[:4] == wl
    last, ll = P.compress(src[batch * hw:], hw, 3, 3, 4)
    assert out[len(out) - len(last):] == last and lens[-1:] == ll


def test_delivery_and_this_librarys_decoder():
    hw = 16384
    src = S.make_input("silesia", 5 * hw - 100, 3)
    s = _session(16, 3, hw, both=True)
    rc, used, out, _ = s.compress(src, 1)
    assert (rc, used) == (A.QZ_OK, len(src))
    assert out == P.compress(src, hw, 3, 3, 16)[0]
    frames = Q.read(out, src, hw)
    assert len(frames) == 5
    rc, used, back = s.decompress(out, len(src))                    # a zstd decode session of this library reads the frames
    assert (rc, used, back) == (A.QZ_OK, len(out), src)
    s.close()
    # QZ_BUF_ERROR: a destination that holds two of three frames, as on the default path
    src3 = src[:3 * hw]
    s = _session(16, 3, hw)
    rc, used, whole, _ = s.compress(src3, 1)
    lens = [f["size"] for f in F.decode_frames(whole)]
    assert rc == A.QZ_OK and len(lens) == 3
    t_in, t_out = s.s.total_in, s.s.total_out
    rc, used, part, _ = s.compress(src3, 1, cap=lens[0] + lens[1] + lens[2] - 1)
    assert (rc, used) == (A.QZ_BUF_ERROR, 2 * hw) and part == whole[:lens[0] + lens[1]]
    assert (s.s.total_in - t_in, s.s.total_out - t_out) == (2 * hw, lens[0] + lens[1])
    rc, used, part, _ = s.compress(src3, 1, cap=3)
    assert (rc, used, part) == (A.QZ_BUF_ERROR, 0, b"")
    s.close()


def test_qzstd_amd_with_a_parse_depth(tmp_path):
    B.build()
    src = S.make_input("records", 300000, 19)
    p = tmp_path / "f"
    p.write_bytes(src)
    r = subprocess.run([B.ZSTD_CLI, "-k", "--parse-depth", "16", "--seq-tables", "--repeat-offsets", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    z = (tmp_path / "f.zst").read_bytes()
    s = _session(16, 3)
    assert s.compress(src, 1)[2] == z
    s.close()
    assert F.decode(z) == src                                       # the strict reader
    zstd_ref.check(z, src)
    p.unlink()
    r = subprocess.run([B.ZSTD_CLI, "--decompress", str(tmp_path / "f.zst")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert p.read_bytes() == src and not (tmp_path / "f.zst").exists()
