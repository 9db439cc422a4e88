"""GPU parity on the trap inputs (tests/deflate_traps.py): Context.deflate_raw in every parse configuration the product
has, compared with libz's own bytes (tests/golden/traps.json, so the oracle is not in the chain) and with the oracle, each
stream decoded back by the GPU inflate.  Needs a real MI355X; the whole file takes about 80 s there (a third of it
building the trap inputs on the host)."""
import hashlib
import json
import os
import subprocess
import sys
import zlib

import pytest

import deflate_traps as T
import oracle_lib as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def sha(b, n=24):
    return hashlib.sha256(b).hexdigest()[:n]


@pytest.fixture(scope="module")
def traps():
    cases = {c.name: c for c in T.all_cases()}
    with open(os.path.join(HERE, "golden", "traps.json")) as f:
        g = json.load(f)
    for name, c in cases.items():
        assert [len(c.data), sha(c.data, 16)] == g["cases"][name], name
    return cases, g["runs"]


@pytest.fixture(scope="module")
def ctx():
    import qatzip_amd
    c = qatzip_amd.Context(0)
    yield c
    c.close()


class Bufs:
    """one source and one destination buffer for all the calls of a test"""
    def __init__(self, ctx, n):
        import qatzip_amd
        self.ctx = ctx
        self.d_src = ctx.alloc(max(n, 1) + 512)
        self.d_dst = ctx.alloc(qatzip_amd.max_deflate_len(max(n, 1), 1024) + 65536)
        self.d_out = ctx.alloc(max(n, 1) + 512)

    def deflate(self, src, hw, level, last):
        self.d_src.upload(src)
        n, crcs = self.ctx.deflate_raw(self.d_src, len(src), hw, level, last, self.d_dst)
        return self.d_dst.download(n).tobytes(), crcs

    def inflate(self, comp, n):
        d_c = self.ctx.alloc(len(comp) + 64)
        d_c.upload(comp)
        _, ol, _ = self.ctx.inflate_stream(d_c, len(comp), self.d_out)
        d_c.free()
        return self.d_out.download(ol).tobytes()

    def free(self):
        self.d_src.free(); self.d_dst.free(); self.d_out.free()


def _runs(runs, cases, levels, fmt="RAW"):
    return [r for r in runs if r[1] == fmt and r[2] in levels]


def _check(b, cases, sel, decode=False, oracle=True):
    for name, fmt, lv, hw, last, olen, osha, ohex in sel:
        src = cases[name].data
        got, crcs = b.deflate(src, hw, lv, last)
        assert len(got) == olen and sha(got) == osha, (name, lv, hw, last, len(got), olen)
        if oracle:
            assert got == O.sw_compress("RAW", src, hw, lv, last=last, cap=len(src) * 9 // 8 + 8192)[2], (name, lv, hw, last)
        for i in range(len(crcs) if src else 0):
            assert int(crcs[i]) == zlib.crc32(src[i * hw:(i + 1) * hw]) & 0xffffffff, (name, i)
        if decode and src and last:
            assert b.inflate(got, len(src)) == src, name


def _maxlen(cases):
    return max(len(c.data) for c in cases.values())


@pytest.mark.parametrize("mode", [("QATZIP_AMD_K1", "pull"), ("QATZIP_AMD_K1", "wide"), ("QATZIP_AMD_K1", None),
                                  ("QATZIP_AMD_DEFLATE", "lane"), ("QATZIP_AMD_K1_OUT", "launch")],
                         ids=["k1_pull", "k1_wide", "auto", "lane", "k1_out_launch"])
def test_level1_traps(ctx, traps, monkeypatch, mode):
    """every level-1 run through K1 (pull), K1w (wide; chunks above 64 KiB stay on K1), the product's own choice, K1b
    and K1 with the waves moving the stream themselves; the product's choice also decodes every stream back"""
    cases, runs = traps
    monkeypatch.delenv("QATZIP_AMD_K1", raising=False)
    if mode[1] is not None:
        monkeypatch.setenv(mode[0], mode[1])
    if mode[0] == "QATZIP_AMD_K1_OUT":
        monkeypatch.setenv("QATZIP_AMD_K1", "pull")
    b = Bufs(ctx, _maxlen(cases))
    try:
        _check(b, cases, _runs(runs, cases, (1,)), decode=mode[1] is None, oracle=mode[1] is None)
    finally:
        b.free()


def test_level1_traps_through_one_workgroup(traps, monkeypatch):
    """QATZIP_AMD_K1_WGS=1: every trap chunk runs through the same workgroup's tables, epoch after epoch"""
    import qatzip_amd
    cases, runs = traps
    monkeypatch.setenv("QATZIP_AMD_K1_WGS", "1")
    monkeypatch.setenv("QATZIP_AMD_K1", "pull")
    c = qatzip_amd.Context(0)
    b = Bufs(c, _maxlen(cases))
    try:
        _check(b, cases, _runs(runs, cases, (1,)), oracle=False)
    finally:
        b.free(); c.close()


def test_level1_traps_with_separate_k2_and_crc_launches():
    """QATZIP_AMD_FUSE=0 is read once per process: a fresh one"""
    code = r'''
import sys
sys.path.insert(0, "tests")
import test_gpu_deflate_traps as G, deflate_traps as T, json, qatzip_amd
cases = {c.name: c for c in T.all_cases()}
runs = json.load(open("tests/golden/traps.json"))["runs"]
c = qatzip_amd.Context(0)
b = G.Bufs(c, G._maxlen(cases))
G._check(b, cases, G._runs(runs, cases, (1,)), oracle=False)
b.free(); c.close()
print("ok")
'''
    env = dict(os.environ, QATZIP_AMD_FUSE="0", QATZIP_AMD_K1="pull")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("level", [2, 3, 4, 5, 6, 7, 8, 9])
def test_other_levels_on_traps(ctx, traps, monkeypatch, level):
    """levels 2-3 through K1b; 4-9 through the lazy kernels and again through K1b (QATZIP_AMD_LAZY=0)"""
    cases, runs = traps
    sel = _runs(runs, cases, (level,))
    b = Bufs(ctx, _maxlen(cases))
    try:
        _check(b, cases, sel, decode=True)
        if level >= 4:
            monkeypatch.setenv("QATZIP_AMD_LAZY", "0")
            _check(b, cases, sel, oracle=False)
    finally:
        b.free()


@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_all_traps_of_a_level_in_one_call(ctx, traps, monkeypatch, level):
    """every trap input of the level back to back in one call (tiled at level 1 to 768+ chunks: well over 1.5 chunks per
    CU of the MI355X's 256, so that the product picks the full K1 launch rather than K1w), against the oracle, decoded
    back"""
    cases, runs = traps
    monkeypatch.delenv("QATZIP_AMD_K1", raising=False)
    names = sorted({r[0] for r in runs if r[2] == level})
    src = b"".join(cases[n].data for n in names)
    if level == 1:
        src = src * max(1, (3 * 256 * 65536) // len(src) + 1)
    b = Bufs(ctx, len(src))
    try:
        got, crcs = b.deflate(src, 65536, level, 1)
        assert got == O.sw_compress("RAW", src, 65536, level, cap=len(src) * 9 // 8 + (1 << 20))[2], level
        assert int(crcs[-1]) == zlib.crc32(src[(len(crcs) - 1) * 65536:]) & 0xffffffff
        assert b.inflate(got, len(src)) == src
    finally:
        b.free()


def test_traps_through_the_api(traps):
    """the GZIP_EXT runs of the goldens through qzCompress (libz wrote those members, header included), and a subset of
    level-1 raw runs as qzCompress2 requests in flight together (the coalesced queue)"""
    import ctypes as C
    import threading
    from qatzip_amd import api as A
    cases, runs = traps
    for name, fmt, lv, hw, last, olen, osha, ohex in (r for r in runs if r[1] == "GZIP_EXT"):
        s = A.Session(A.QZ_DEFLATE_GZIP_EXT, hw, comp_lvl=lv)
        rc, used, out, _ = s.compress(cases[name].data, last=last)
        s.close()
        assert rc == A.QZ_OK and len(out) == olen and sha(out) == osha, (name, lv, hw, len(out), olen)
    sel = [r for r in runs if r[1] == "RAW" and r[2] == 1 and r[3] == 65536 and r[4] == 1 and len(cases[r[0]].data) <= 65536][::3]
    sess = A.Session(A.QZ_DEFLATE_RAW, 65536, comp_lvl=1)
    L = sess.L
    bins = [C.create_string_buffer(cases[r[0]].data, max(1, len(cases[r[0]].data))) for r in sel]
    bouts = [C.create_string_buffer(len(cases[r[0]].data) * 9 // 8 + 4096) for r in sel]
    res = [A.QzResult() for _ in sel]
    done, order = threading.Event(), []

    def on_done(p):
        order.append(p.contents.cb_tag)
        if len(order) == len(sel):
            done.set()
        return 0
    cb = A.QzAsyncCallback(on_done)
    for i, r in enumerate(sel):
        res[i].cb_tag = i + 1; res[i].src_len = len(cases[r[0]].data); res[i].dest_len = len(bouts[i])
        assert L.qzCompress2(C.byref(sess.s), bins[i], bouts[i], cb, C.byref(res[i])) == A.QZ_OK
    assert done.wait(600)
    for i, r in enumerate(sel):
        out = bouts[i].raw[:res[i].dest_len]
        assert res[i].status == A.QZ_OK and len(out) == r[5] and sha(out) == r[6], r[0]
    sess.close()
    assert len(sel) > 50
