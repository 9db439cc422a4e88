"""GPU parity on the LZ4 trap inputs (tests/lz4_traps.py): both routes of Context.lz4_compress_frames - the kernel with its
table in LDS and the persistent pull kernel - with equal-size traps as the frames of one call, the linked-block kernel,
and the session API, every frame compared with liblz4 1.9.3's own bytes (tests/golden/lz4_traps/index.json: the oracle is
not in the chain).  Needs a real MI355X."""
import contextlib
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lz4_traps as T
from qatzip_amd import api as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def traps():
    tr = T.all_traps()
    with open(os.path.join(HERE, "golden", "lz4_traps", "index.json")) as f:
        idx = {e["name"]: e for e in json.load(f)["traps"]}
    for t in tr:
        assert (len(t.data), sha(t.data)) == (idx[t.name]["n"], idx[t.name]["input_sha256"]), t.name
        assert idx[t.name]["live"]
    return tr, idx


@pytest.fixture(scope="module")
def ctx():
    import qatzip_amd
    c = qatzip_amd.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def wpc(value):
    old = os.environ.get("QATZIP_AMD_LZ4_WPC")
    try:
        if value is None:
            os.environ.pop("QATZIP_AMD_LZ4_WPC", None)
        else:
            os.environ["QATZIP_AMD_LZ4_WPC"] = value
        yield
    finally:
        if old is None:
            os.environ.pop("QATZIP_AMD_LZ4_WPC", None)
        else:
            os.environ["QATZIP_AMD_LZ4_WPC"] = old


def cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a fresh process: torch brings a HIP runtime of its
    own, which finds no device in a process where the package's runtime already holds it"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


def pinned(idx, t, out):
    return len(out) == idx[t.name]["frame_len"] and sha(out) == idx[t.name]["frame_sha256"]


def one_call(ctx, src, fs):
    """src (numpy bytes) as frames of fs bytes -> the frames, each as bytes"""
    n = int(src.size)
    nfr = max(1, (n + fs - 1) // fs)
    d_src = ctx.alloc(max(n, 1)); d_dst = ctx.alloc(n + nfr * 64 + 4096)
    try:
        if n:
            d_src.upload(src)
        total, lens = ctx.lz4_compress_frames(d_src, n, d_dst, fs)
        assert int(lens.sum()) == total
        comp = d_dst.download(total)
    finally:
        d_src.free(); d_dst.free()
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    return [comp[offs[i]:offs[i + 1]].tobytes() for i in range(nfr)]


def test_lds_table_route_on_every_block_trap(ctx, traps):
    """per trap size one call whose frames are that size's traps, by the one-wave-per-frame kernel (QATZIP_AMD_LZ4_WPC=0)"""
    tr, idx = traps
    for fs, group in T.by_size(tr).items():
        src = np.frombuffer(b"".join(t.data for t in group), np.uint8)
        with wpc("0"):
            outs = one_call(ctx, src, fs or 65536)
        assert len(outs) == len(group)
        for t, out in zip(group, outs):
            assert pinned(idx, t, out), (t.name, t.aim, len(out), idx[t.name]["frame_len"])


def test_pull_route_on_every_block_trap_every_frame_compared(ctx, traps):
    """the same per-size calls with the traps cycled until the call has more than eight frames per CU: the persistent pull
    kernel (epoch-tagged tables reused from frame to frame, register windows, staged output).  Every frame is compared.  The
    4096-byte class ends in a shorter trap: the ragged tail is the only way an odd size reaches this kernel."""
    tr, idx = traps
    cus = cu_count()
    want = 8 * cus + 1
    short = next(t for t in tr if len(t.data) == 700)
    for fs, group in T.by_size(tr).items():
        if fs == 0:
            continue
        one = np.frombuffer(b"".join(t.data for t in group), np.uint8)
        reps = -(-want // len(group))
        src = np.tile(one, reps)
        names = group * reps
        if fs == 4096:
            src = np.concatenate([src[:-fs], np.frombuffer(short.data, np.uint8)])
            names = names[:-1] + [short]
        with wpc(None):
            outs = one_call(ctx, src, fs)
        assert len(outs) == len(names) > 8 * cus
        good = {}
        for i, (t, out) in enumerate(zip(names, outs)):
            if t.name not in good:
                assert pinned(idx, t, out), (fs, i, t.name, t.aim, len(out), idx[t.name]["frame_len"])
                good[t.name] = out
            else:
                assert out == good[t.name], (fs, i, t.name)


def test_linked_traps_by_the_kernel_and_the_session(ctx, traps):
    tr, idx = traps
    linked = [t for t in tr if t.mode == "linked"]
    s = A.Session(lz4=True)
    assert s.rc_setup == A.QZ_OK
    for t in linked:
        n = len(t.data)
        d_src = ctx.alloc(n); d_src.upload(np.frombuffer(t.data, np.uint8))
        d_dst = ctx.alloc(n + n // 255 + 4096)
        total = ctx.lz4_compress_linked(d_src, n, d_dst)
        out = d_dst.download(total).tobytes()
        d_src.free(); d_dst.free()
        assert pinned(idx, t, out), (t.name, t.aim)
        rc, used, out, _ = s.compress(t.data, 1, cap=n + n // 255 + 4096)
        assert rc == A.QZ_OK and used == n and pinned(idx, t, out), (t.name, "session")
    s.close()


def test_block_traps_through_the_session(traps):
    """two traps per family (the first and the last of each) through qzCompress"""
    tr, idx = traps
    s = A.Session(lz4=True)
    assert s.rc_setup == A.QZ_OK
    count = 0
    for fam in T.FAMILIES:
        ts = [t for t in tr if t.family == fam and t.mode == "block" and len(t.data) > 0]
        for t in ([ts[0], ts[-1]] if ts else []):
            n = len(t.data)
            rc, used, out, _ = s.compress(t.data, 1, cap=n + n // 255 + 4096)
            assert rc == A.QZ_OK and used == n and pinned(idx, t, out), (t.name, t.aim)
            count += 1
    s.close()
    assert count >= 12
