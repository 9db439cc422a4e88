"""GPU parity on the trap inputs of Kzp, the hash-chain lazy parse of zstd sessions (tests/zstd_parse_traps.py): every trap at
its own hw_buff_sz, mini_match and depth through a session and through the device layer's call.  The serial model does not
run here; tests/golden/zstd_parse_traps/index.json carries its answers (made by tests/golden/gen_zstd_parse_traps.py, which
took nothing from the kernels before the model agreed): the SHA-256 of the model's sequence list, the repeat codes it
predicts, and the frames' lengths and SHA-256 under sequence flags 0 and 3.  The strict reader takes the sequences out of the
GPU's own frames.  Needs a real MI355X.  The CPU twin, with the model, every trap's check and the label coverage, is
tests/test_sim_zstd_parse_traps.py."""
import hashlib
import json
import os

import pytest

import zstd_parse_traps as T
import zstd_seq_sim as Q
import qatzip_amd
from qatzip_amd import api as A
from qatzip_amd._lib import zstd_bound

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def sha(b):
    return hashlib.sha256(b).hexdigest()


def seq_sha(seqs):
    return sha(json.dumps([list(s) for s in seqs], separators=(",", ":")).encode())


@pytest.fixture(scope="module")
def traps():
    tr = T.all_traps()
    with open(os.path.join(HERE, "golden", "zstd_parse_traps", "index.json")) as f:
        idx = {e["name"]: e for e in json.load(f)["traps"]}
    assert [t.name for t in tr] == list(idx)
    for t in tr:
        e = idx[t.name]
        assert (len(t.data), sha(t.data), t.hw_buff_sz, t.mini_match, t.depth) == (e["n"], e["input_sha256"], e["hw_buff_sz"], e["mini_match"], e["depth"]), t.name
    return tr, idx


@pytest.fixture(scope="module")
def ctx():
    c = qatzip_amd.Context(0)
    yield c
    c.close()


def device_frames(ctx, src, hw, mm, flags, depth):
    """qzd_zstd_compress_frames_parse -> (stream, per-frame lengths)"""
    d_src = ctx.alloc(max(len(src), 1)); d_src.upload(src)
    d_dst = ctx.alloc(zstd_bound(len(src), hw) + 64)
    try:
        n, lens = ctx.zstd_compress_frames(d_src, len(src), d_dst, hw, mm, 1, dst_cap=zstd_bound(len(src), hw), seq_flags=flags, parse_depth=depth)
        out = d_dst.download(n).tobytes()
    finally:
        d_src.free(); d_dst.free()
    assert int(lens.sum()) == n
    return out, [int(x) for x in lens]


def pinned(e, flags, out):
    return (len(out), sha(out)) == (e["frames"][str(flags)]["len"], e["frames"][str(flags)]["sha256"])


def holds_the_models_sequences(t, e, out, flags):
    """the strict reader (and libzstd, where it loads) on the GPU's frame: the sequences have the model's SHA-256, the repeat
    codes met are the predicted ones"""
    f = Q.read(out, t.data, t.hw_buff_sz)[0]
    reps = sorted(x for x in f["tally"] if x.startswith("rep:"))
    assert ("block:compressed" in f["tally"]) == e["frames"][str(flags)]["compressed"], t.name
    if "block:compressed" in f["tally"]:
        assert (seq_sha([tuple(s) for s in f["sequences"]]), len(f["sequences"])) == (e["seq_sha256"], e["nseq"]), (t.name, t.aim)
        assert reps == (e["rep"] if flags & 2 else []), (t.name, t.aim)
    else:
        assert reps == [] and not f["sequences"], t.name


def test_every_trap_through_a_session(traps):
    """qzSetupSessionZstdAMD, set_zstd_parse, set_zstd_seq(3), qzCompress: one session per (hw_buff_sz, mini_match), the depth
    set again for every trap"""
    tr, idx = traps
    sessions = {}
    try:
        for t in tr:
            key = (t.hw_buff_sz, t.mini_match)
            if key not in sessions:
                s = sessions[key] = A.Session(zstd=True, hw_buff_sz=t.hw_buff_sz, mini_match=t.mini_match)
                assert s.rc_setup == A.QZ_OK and s.set_zstd_seq(3) == A.QZ_OK
            s = sessions[key]
            assert s.set_zstd_parse(t.depth) == A.QZ_OK
            rc, used, out, _ = s.compress(t.data, 1)
            assert (rc, used) == (A.QZ_OK, len(t.data)), t.name
            assert pinned(idx[t.name], 3, out), (t.name, t.aim, len(out), idx[t.name]["frames"]["3"]["len"])
    finally:
        for s in sessions.values():
            s.close()
    assert len(sessions) >= 10


@pytest.mark.parametrize("family", T.FAMILIES)
def test_every_trap_through_the_device_call(ctx, traps, family):
    """qzd_zstd_compress_frames_parse under flags 3: the pinned frame, the model's sequences, the predicted repeat codes"""
    tr, idx = traps
    todo = [t for t in tr if t.family == family]
    assert todo
    for t in todo:
        out, lens = device_frames(ctx, t.data, t.hw_buff_sz, t.mini_match, 3, t.depth)
        assert lens == [len(out)], t.name
        holds_the_models_sequences(t, idx[t.name], out, 3)
        assert pinned(idx[t.name], 3, out), (t.name, t.aim)


def test_a_subset_under_flags_0(ctx, traps):
    """the first two block-sized traps of every family without sequence flags: the same sequences, no repeat code, the frame
    pinned for flags 0"""
    tr, idx = traps
    count = 0
    for fam in T.FAMILIES:
        for t in [t for t in tr if t.family == fam and len(t.data) <= 65536 and idx[t.name]["frames"]["0"]["compressed"]][:2]:
            out, _ = device_frames(ctx, t.data, t.hw_buff_sz, t.mini_match, 0, t.depth)
            holds_the_models_sequences(t, idx[t.name], out, 0)
            assert pinned(idx[t.name], 0, out), (t.name, t.aim)
            count += 1
    assert count >= len(T.FAMILIES)


def test_traps_as_the_chunks_of_one_call(ctx, traps):
    """the 1024-byte traps of one mini_match and depth as one call at hw_buff_sz 1024, and repeated to more than 300 chunks -
    several workgroups in P1 .. P3, P4's pull counter in play: every chunk's frame is that of its trap alone"""
    tr, idx = traps
    group = T.independent_traps()
    assert len(group) >= 16
    hw, mm, depth = T.CI
    for reps in (1, 300 // len(group) + 1):
        names = group * reps
        assert reps == 1 or len(names) >= 300
        out, lens = device_frames(ctx, b"".join(t.data for t in names), hw, mm, 3, depth)
        assert len(lens) == len(names)
        pos = 0
        for i, (t, ln) in enumerate(zip(names, lens)):
            assert pinned(idx[t.name], 3, out[pos:pos + ln]), (i, t.name)
            pos += ln
        assert pos == len(out)
