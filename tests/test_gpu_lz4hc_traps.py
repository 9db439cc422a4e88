"""GPU parity on the LZ4-HC trap inputs (tests/lz4hc_traps.py): Context.lz4_compress_frames at levels 3-8 with equal-size
traps as the frames of one call, the same behind the hardware path's header, Context.lz4_compress_linked and the session API
on the linked traps, and one call of more blocks than a round of lz4hc_impl holds - every frame compared with liblz4 1.9.3's
own bytes (tests/golden/lz4hc_traps/index.json: no oracle in the chain).  Needs a real MI355X.  The CPU twin, with the
liveness of every trap and the label census, is tests/test_sim_lz4hc_traps.py."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import lz4hc_traps as T
from qatzip_amd import api as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HW_HEAD = bytes([0x04, 0x22, 0x4D, 0x18, 0x4C, 0x40])


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def traps():
    tr = T.all_traps()
    with open(os.path.join(HERE, "golden", "lz4hc_traps", "index.json")) as f:
        idx = {e["name"]: e for e in json.load(f)["traps"]}
    for t in tr:
        assert (len(t.data), sha(t.data)) == (idx[t.name]["n"], idx[t.name]["input_sha256"]), t.name
        assert all(idx[t.name]["levels"][str(lvl)]["live"] for lvl in t.levels), t.name
    return tr, idx


@pytest.fixture(scope="module")
def ctx():
    import qatzip_amd
    c = qatzip_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sessions():
    ss = {lvl: A.Session(lz4=True, comp_lvl=lvl) for lvl in T.LEVELS}
    assert all(s.rc_setup == A.QZ_OK for s in ss.values())
    yield ss
    for s in ss.values():
        s.close()


def pinned(idx, t, lvl, out):
    e = idx[t.name]["levels"][str(lvl)]
    return len(out) == e["frame_len"] and sha(out) == e["frame_sha256"]


def one_call(ctx, src, fs, level, hw=False):
    """src (numpy bytes, not empty) as frames of fs bytes -> the frames, each as bytes"""
    n = int(src.size)
    nfr = (n + fs - 1) // fs
    d_src = ctx.alloc(n); d_dst = ctx.alloc(n + (nfr + n // 65536 + 1) * 64 + 4096)
    try:
        d_src.upload(src)
        total, lens = ctx.lz4_compress_frames(d_src, n, d_dst, fs, level=level, hw=hw)
        assert int(lens.sum()) == total
        comp = d_dst.download(total)
    finally:
        d_src.free(); d_dst.free()
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    return [comp[offs[i]:offs[i + 1]].tobytes() for i in range(nfr)]


def hw_equals_pin(out, fs, e):
    """a frame behind qzLZ4HeaderGen's header: the header, then the pinned frame from byte 15 on (its own header rebuilt)"""
    if out[:6] != HW_HEAD or out[6:14] != fs.to_bytes(8, "little") or len(out) != e["frame_len"]:
        return False
    desc = bytes([0x6C if fs <= 65536 else 0x4C, 0x40]) + fs.to_bytes(8, "little")
    return sha(b"\x04\x22\x4d\x18" + desc + bytes([(T.xxh32(desc) >> 8) & 0xff]) + out[15:]) == e["frame_sha256"]


@pytest.mark.parametrize("lvl", T.LEVELS)
def test_block_traps_one_call_per_size(ctx, traps, lvl):
    """per size class one call whose frames are that class's traps, plain and behind the hardware path's header (the empty
    input has no frame size to call with: test_block_traps_through_the_session runs it)"""
    tr, idx = traps
    for fs, group in T.by_size(tr).items():
        if fs == 0:
            continue
        todo = [t for t in group if lvl in t.levels]
        src = np.frombuffer(b"".join(t.data for t in todo), np.uint8)
        outs = one_call(ctx, src, fs, lvl)
        assert len(outs) == len(todo)
        for t, out in zip(todo, outs):
            assert pinned(idx, t, lvl, out), (t.name, lvl, t.aim, len(out), idx[t.name]["levels"][str(lvl)]["frame_len"])
        for t, out in zip(todo, one_call(ctx, src, fs, lvl, hw=True)):
            assert hw_equals_pin(out, fs, idx[t.name]["levels"][str(lvl)]), (t.name, lvl, "hardware-path header")


def test_linked_traps_by_the_kernel_the_session_and_the_hardware_path(ctx, sessions, traps):
    tr, idx = traps
    linked = [t for t in tr if T.is_linked(t)]
    assert len(linked) >= 8
    for t in linked:
        n = len(t.data)
        src = np.frombuffer(t.data, np.uint8)
        for lvl in t.levels:
            e = idx[t.name]["levels"][str(lvl)]
            d_src = ctx.alloc(n); d_src.upload(src)
            d_dst = ctx.alloc(n + n // 255 + 4096)
            try:
                total = ctx.lz4_compress_linked(d_src, n, d_dst, level=lvl)
                out = d_dst.download(total).tobytes()
            finally:
                d_src.free(); d_dst.free()
            assert pinned(idx, t, lvl, out), (t.name, lvl, t.aim)
            rc, used, out, _ = sessions[lvl].compress(t.data, 1, cap=n + n // 255 + 4096)
            assert rc == A.QZ_OK and used == n and pinned(idx, t, lvl, out), (t.name, lvl, "session")
            # hw_buff_sz 65536: a frame per 64 KB chunk; 262144: one chunk, and above 64 KB liblz4's own FLG is 0x4C too
            outs = one_call(ctx, src, 65536, lvl, hw=True)
            assert len(outs) == len(e["hw65536"])
            for i, (out, ch) in enumerate(zip(outs, e["hw65536"])):
                piece = min(65536, n - i * 65536)
                assert out[:6] == HW_HEAD and out[6:14] == piece.to_bytes(8, "little"), (t.name, lvl, i)
                assert len(out) == 15 + ch["len"] and sha(out[15:]) == ch["sha"], (t.name, lvl, i)
            outs = one_call(ctx, src, 262144, lvl, hw=True)
            assert len(outs) == 1 and pinned(idx, t, lvl, outs[0]), (t.name, lvl, "hw_buff_sz 262144")


def test_block_traps_through_the_session(sessions, traps):
    """two traps per family (the first and the last of each) and the empty input through qzCompress, at every level"""
    tr, idx = traps
    count = 0
    for fam in T.FAMILIES:
        ts = [t for t in tr if t.family == fam and not T.is_linked(t) and len(t.data) > 0]
        for t in ([ts[0], ts[-1]] if ts else []) + ([x for x in tr if len(x.data) == 0] if fam == "E" else []):
            n = len(t.data)
            for lvl in t.levels:
                rc, used, out, _ = sessions[lvl].compress(t.data, 1, cap=n + n // 255 + 4096)
                assert rc == A.QZ_OK and used == n and pinned(idx, t, lvl, out), (t.name, lvl, t.aim)
            count += 1
    assert count >= 10


def test_more_blocks_than_one_round_holds(ctx, traps):
    """the 256-byte class cycled until the call has more blocks than a round of lz4hc_impl (QZD_HC_BATCH): the second round
    reuses the head tables, the chain distances and the slots of the first.  Every repeat equals its first occurrence, and
    that one is the pinned frame."""
    tr, idx = traps
    with open(os.path.join(os.path.dirname(HERE), "qatzip_amd", "csrc", "qzd_device.hip")) as f:
        batch = int(re.search(r"#define\s+QZD_HC_BATCH\s+(\d+)u", f.read()).group(1))
    assert 1024 <= batch <= 8192
    fs = 256
    group = T.by_size(tr)[fs]
    reps = batch // len(group) + 2
    names = (group * reps)[:batch + len(group) + 1]
    assert len(names) > batch
    src = np.tile(np.frombuffer(b"".join(t.data for t in group), np.uint8), reps)[:len(names) * fs]
    for lvl in (3, 8):
        outs = one_call(ctx, src, fs, lvl)
        assert len(outs) == len(names)
        first = {}
        for i, (t, out) in enumerate(zip(names, outs)):
            if t.name not in first:
                assert pinned(idx, t, lvl, out), (i, t.name, lvl)
                first[t.name] = out
            else:
                assert out == first[t.name], (i, t.name, lvl)
