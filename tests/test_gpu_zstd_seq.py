"""Zstd sessions with qzSetSessionZstdSeqAMD (include/qzamd_zstd_seq.h) on the GPU: sessions and the device layer's _ex
calls give the bytes the CPU emulator pinned in tests/golden/zstd_seq/index.json (made by tests/golden/gen_zstd_seq.py, where
every stream was also decoded by libzstd); flags 0 is the writer as it was; delivery, a round trip on one session, and
qzstd-amd with the two options.  Every frame is read by the strict reader of whole frames, tests/zstd_full_format.py."""
import ctypes as C
import hashlib
import subprocess

import numpy as np
import pytest

import zstd_format as Z
import zstd_full_format as F
import zstd_ref
import zstd_seq_sim as Q
import zstd_sim as S
import qatzip_amd
import qatzip_amd.build as B
from qatzip_amd import api as A
from qatzip_amd._lib import zstd_bound

pytestmark = pytest.mark.gpu


def _sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def ctx():
    c = qatzip_amd.Context(0)
    yield c
    c.close()


def _session(flags, hw=65536, mm=3, both=False):
    s = A.Session(zstd=not both, zstd_dec=A.QZ_DIR_BOTH if both else None, hw_buff_sz=hw, mini_match=mm)
    assert s.rc_setup == A.QZ_OK
    if flags is not None:
        assert s.set_zstd_seq(flags) == A.QZ_OK
    return s


def device_frames(ctx, src, hw, mm, flags):
    d_src = ctx.alloc(max(len(src), 1)); d_src.upload(src)
    d_dst = ctx.alloc(zstd_bound(len(src), hw) + 64)
    n, lens = ctx.zstd_compress_frames(d_src, len(src), d_dst, hw, mm, 1, dst_cap=zstd_bound(len(src), hw), seq_flags=flags)
    out = d_dst.download(n).tobytes()
    d_src.free(); d_dst.free()
    assert int(lens.sum()) == n
    return out, [int(x) for x in lens]


def device_encode(ctx, frames, flags):
    lits, seqs, desc = S.pack_frames(frames)
    d_l = ctx.alloc(len(lits) + 16); d_l.upload(lits + b"\0")
    d_s = ctx.alloc(seqs.nbytes + 16); d_s.upload(np.concatenate([seqs, np.zeros(3, np.uint32)]).tobytes())
    cap = sum(min(f[0], Z.MAX_BLOCK) + 12 for f in frames)
    d_dst = ctx.alloc(cap + 64)
    rc, n, lens = ctx.zstd_encode_frames(d_l, d_s, desc, d_dst, dst_cap=cap, seq_flags=flags)
    out = d_dst.download(n).tobytes() if n else b""
    d_l.free(); d_s.free(); d_dst.free()
    return rc, out, [int(x) for x in lens]


def test_sessions_reproduce_the_pinned_index(ctx):
    """qzCompress on a session with the case's flags; the cases with other chunk sizes go through the device layer too"""
    cases = Q.index()["cases"]
    assert len(cases) >= 24
    sessions = {}
    for c in cases:
        src = S.make_input(c["kind"], c["n"], c["seed"])
        assert _sha(src) == c["in_sha"], c
        key = (c["flags"], c["hw_buff_sz"], c["mini_match"])
        if key not in sessions:
            sessions[key] = _session(*key)
        rc, used, out, _ = sessions[key].compress(src, 1)
        assert (rc, used) == (A.QZ_OK, len(src)), c
        assert (len(out), _sha(out)) == (c["out_len"], c["out_sha"]), c
    for s in sessions.values():
        s.close()
    c = next(x for x in cases if x["kind"] == "records" and x["flags"] == 3 and x["n"] == 70001 and x["mini_match"] == 3)
    src = S.make_input(c["kind"], c["n"], c["seed"])
    out, lens = device_frames(ctx, src, 65536, 3, 3)
    assert (len(out), _sha(out)) == (c["out_len"], c["out_sha"])
    frames = Q.read(out, src, 65536)
    assert [f["sequences"] for f in frames] == S.expected_sequences(src, 65536, 3)
    assert "of:fse" in frames[0]["tally"] and any(t.startswith("rep:") for t in frames[0]["tally"])


def test_edge_frames_equal_the_pins_and_the_emulator(ctx):
    names = sorted(Q.EDGES) + sorted(Q.REP)
    both = dict(Q.EDGES, **Q.REP)
    idx = Q.index()["edges"]
    for flags in (1, 2, 3):
        rc, out, lens = device_encode(ctx, [both[k] for k in names], flags)
        assert rc == 0 and sum(lens) == len(out)
        pos = 0
        for k, ln in zip(names, lens):
            one = out[pos:pos + ln]
            pos += ln
            assert [ln, _sha(one)] == idx[str(flags)][k], (flags, k)
        if flags == 3:
            f = Q.read(out[:lens[0]], S.rebuild(both[names[0]]), both[names[0]][0])[0]
            assert f["sequences"] == both[names[0]][1]
            rc, sim, _ = Q.encode([both[k] for k in names], 3)
            assert rc == 0 and sim == out


def test_flags_0_gives_the_old_bytes(ctx):
    old = S.index()["cases"]
    c = next(x for x in old if x["kind"] == "silesia" and x["n"] == 70001 and x["mini_match"] == 3)
    src = S.make_input(c["kind"], c["n"], c["seed"])
    s = _session(3)
    rc, used, out3, _ = s.compress(src, 1)
    assert rc == A.QZ_OK and len(out3) < c["out_len"]
    assert s.set_zstd_seq(0) == A.QZ_OK
    rc, used, out, _ = s.compress(src, 1)
    assert (rc, used) == (A.QZ_OK, len(src)) and (len(out), _sha(out)) == (c["out_len"], c["out_sha"])
    s.close()
    assert device_frames(ctx, src, 65536, 3, 0)[0] == out == device_frames(ctx, src, 65536, 3, None)[0]
    names = ("count127", "count128", "huf1024", "ll65536")
    assert device_encode(ctx, [S.EDGES[k] for k in names], 0) == device_encode(ctx, [S.EDGES[k] for k in names], None)
    # a bit above 3: QZD_ERR_PARAM, nothing written
    rc, out, _ = device_encode(ctx, [S.EDGES["rle"]], 4)
    assert rc == -1 and out == b""
    d = ctx.alloc(4096); big = ctx.alloc(zstd_bound(1000, 1024) + 64)
    ol = C.c_uint64(7)
    assert ctx.L.qzd_zstd_compress_frames_ex(ctx.h, d.ptr, 1000, 1024, 3, 1, big.ptr, big.nbytes, C.byref(ol), None, 4) == -1
    d.free(); big.free()


def test_round_trip_on_one_session_and_delivery():
    hw = 16384
    src = S.make_input("silesia", 5 * hw - 100, 3)
    s = _session(3, hw, both=True)
    rc, used, out, _ = s.compress(src, 1)
    assert (rc, used) == (A.QZ_OK, len(src))
    assert s.L.qzMaxCompressedLength(len(src), C.byref(s.s)) == len(src) + 5 * 12
    frames = Q.read(out, src, hw)
    assert len(frames) == 5 and [f["sequences"] for f in frames] == S.expected_sequences(src, hw, 3)
    assert any("fse" in Q.modes(f).values() for f in frames)
    rc, used, back = s.decompress(out, len(src))
    assert (rc, used, back) == (A.QZ_OK, len(out), src)
    s.close()
    # QZ_BUF_ERROR: a destination that holds two of three frames
    src3 = src[:3 * hw]
    s = _session(3, hw)
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


def test_qzstd_amd_with_the_two_options(tmp_path):
    B.build()
    src = S.make_input("records", 200 * 1024, 19)
    p = tmp_path / "f"
    p.write_bytes(src)
    r = subprocess.run([B.ZSTD_CLI, "-k", "--seq-tables", "--repeat-offsets", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    z = (tmp_path / "f.zst").read_bytes()
    s = _session(3)
    assert s.compress(src, 1)[2] == z
    s.close()
    zstd_ref.check(z, src)
    p.unlink()
    r = subprocess.run([B.ZSTD_CLI, "--decompress", str(tmp_path / "f.zst")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert p.read_bytes() == src and not (tmp_path / "f.zst").exists()
    # without the options: the file a session with flags 0 writes, which --decompress reads as well
    r = subprocess.run([B.ZSTD_CLI, "-k", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    z0 = (tmp_path / "f.zst").read_bytes()
    s = _session(0)
    assert s.compress(src, 1)[2] == z0 and len(z) < len(z0)
    s.close()
    r = subprocess.run([B.ZSTD_CLI, "--decompress", "-o", str(tmp_path / "g"), str(tmp_path / "f.zst")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and (tmp_path / "g").read_bytes() == src
