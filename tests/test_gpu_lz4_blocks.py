"""GPU: LZ4 frames of independent blocks a wave per block (qzk_lz4.h K5b) against the one-wave kernel and against
tests/golden/lz4_blocks - frames liblz4 1.9.3 wrote, and hand-built ones with what its LZ4F_decompress answered
(tests/golden/gen_lz4_blocks.py): block checksums are verified, a match that reaches in front of an independent block is
refused, and the verdict does not depend on the route.  The CPU twin is tests/test_sim_lz4_blocks.py."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import datagen
import lz4_frame_writer as W
from qatzip_amd import api as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "lz4_blocks")
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_lz4_blocks  # noqa: E402

with open(os.path.join(GOLD, "index.json")) as f:
    INDEX = json.load(f)
with open(os.path.join(HERE, "golden", "lz4_linked", "index.json")) as f:
    LINKED = json.load(f)["frames"]
GUARD = 67


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@pytest.fixture(scope="module")
def ctx():
    import qatzip_amd
    c = qatzip_amd.Context(0)
    yield c
    c.lz4_decode_route("auto")
    c.close()


@pytest.fixture(scope="module")
def verdict_frames():
    return {name: (fr, short) for name, fr, short in gen_lz4_blocks.verdict_frames()}


def decode(ctx, frames, caps, route, phase=5):
    """the frames as the segments of ONE call; outputs `phase` bytes off a 16-byte boundary, GUARD bytes of 0xA5 behind every
    out_cap -> (results, [output of each good segment]); the guards are checked here"""
    comp = b"".join(frames)
    d_c = ctx.alloc(len(comp)); d_c.upload(comp)
    segs, io, oo = [], 0, phase
    for fr, cap in zip(frames, caps):
        segs.append((io, oo, len(fr), cap))
        io += len(fr); oo += cap + GUARD
    d_o = ctx.alloc(oo + 16); d_o.upload(np.full(oo + 16, 0xA5, np.uint8))
    try:
        res = ctx.lz4_decompress_frames(d_c, d_o, segs, route=route)
        out = d_o.download(oo + 16)
    finally:
        d_c.free(); d_o.free()
    assert (out[:phase] == 0xA5).all()
    outs = []
    for i, (_, o, _, cap) in enumerate(segs):
        assert (out[o + cap:o + cap + GUARD] == 0xA5).all(), ("a store beyond out_cap", i, route)
        if res[i]["status"] == -2 and route != "wave":
            assert (out[o:o + cap] == 0xA5).all(), ("output of a frame that does not fit", i)
        outs.append(out[o:o + int(res[i]["out_len"])].tobytes() if res[i]["status"] == 0 else None)
    return res, outs


@pytest.mark.parametrize("v", INDEX["verdicts"], ids=lambda v: v["name"])
def test_verdicts_on_both_routes(ctx, verdict_frames, v):
    fr, short = verdict_frames[v["name"]]
    assert _sha(fr) == v["sha"]
    ok = v["liblz4"] == "OK"
    cap = v["out_len"] - short if ok else 80000
    got = {}
    for route in ("blocks", "wave"):
        res, outs = decode(ctx, [fr], [cap], route)
        r = res[0]
        if ok and not short:
            assert r["status"] == 0 and r["in_used"] == len(fr) and r["out_len"] == v["out_len"], (route, r)
            assert _sha(outs[0]) == v["out_sha"], route
        else:
            assert r["status"] != 0, (route, r)
        got[route] = (int(r["status"]), outs[0])
    assert got["blocks"] == got["wave"], v["name"]
    if short:
        assert got["blocks"][0] == -2


@pytest.mark.parametrize("f", INDEX["files"], ids=lambda f: f["file"])
def test_liblz4_frames_on_both_routes(ctx, f):
    with open(os.path.join(GOLD, f["file"]), "rb") as fh:
        fr = fh.read()
    assert _sha(fr) == f["out_sha"]
    src = datagen.gen_bytes(f["kind"], f["n"], f["seed"])
    for route in ("blocks", "wave"):
        res, outs = decode(ctx, [fr], [f["n"] + (route == "wave")], route, phase=11)
        assert res[0]["status"] == 0 and res[0]["in_used"] == len(fr) and res[0]["out_len"] == f["n"], (route, res[0])
        assert outs[0] == src, route


def test_verdicts_through_qzdecompress(verdict_frames):
    s = A.Session(lz4=True)
    assert s.rc_setup == A.QZ_OK
    try:
        for v in INDEX["verdicts"]:
            fr, short = verdict_frames[v["name"]]
            ok = v["liblz4"] == "OK"
            rc, used, back = s.decompress(fr, v["out_len"] - short if ok else 80000)
            if ok and not short:
                assert rc == A.QZ_OK and used == len(fr) and _sha(back) == v["out_sha"], v["name"]
            else:
                assert rc != A.QZ_OK, v["name"]
    finally:
        s.close()


def test_mixed_segments_in_one_call(ctx, verdict_frames):
    """four 64 KB single-block frames, a two-block independent frame, a linked frame, the 8000-block frame and a frame with a
    bad block checksum in one call, every output at an address that is no multiple of 16"""
    parts = [datagen.gen_bytes(k, 65536, 40 + i) for i, k in enumerate(("text", "silesia", "rand", "records"))]
    src = b"".join(parts)
    d_s = ctx.alloc(len(src)); d_s.upload(src)
    d_d = ctx.alloc(len(src) + 4 * 64 + 64)
    total, lens = ctx.lz4_compress_frames(d_s, len(src), d_d, 65536)
    comp = d_d.download(total).tobytes()
    d_s.free(); d_d.free()
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    frames = [comp[offs[i]:offs[i + 1]] for i in range(4)]
    want = list(parts)
    by = {v["name"]: v for v in INDEX["verdicts"]}
    lk = next(x for x in LINKED if x["n"] > 131072)
    with open(os.path.join(HERE, "golden", "lz4_linked", lk["file"]), "rb") as fh:
        linked = fh.read()
    frames += [verdict_frames["dict_id"][0], linked, verdict_frames["8000_stored_blocks"][0], verdict_frames["three_blocks_nocc_badsum1"][0]]
    want += [by["dict_id"]["out_sha"], datagen.gen_bytes(lk["kind"], lk["n"], lk["seed"]), by["8000_stored_blocks"]["out_sha"], None]
    caps = [65536] * 4 + [by["dict_id"]["out_len"], lk["n"], by["8000_stored_blocks"]["out_len"], 80000]
    seen = {}
    for route in ("auto", "wave"):
        res, outs = decode(ctx, frames, caps, route, phase=7)
        for i, w in enumerate(want):
            if w is None:
                assert res[i]["status"] == -1, (route, i)
                continue
            assert res[i]["status"] == 0 and res[i]["in_used"] == len(frames[i]), (route, i, res[i])
            assert (_sha(outs[i]) if isinstance(w, str) else outs[i]) == w, (route, i)
        seen[route] = [(int(r["status"]), int(r["in_used"]), int(r["out_len"])) for r in res if r["status"] == 0]
    assert seen["auto"] == seen["wave"]


@pytest.fixture(scope="module")
def blocks_16mib(ctx):
    """16 MiB as 256 block bodies of the library's own 64 KB software frames (other tests pin those bytes to liblz4)"""
    base = np.concatenate([datagen.gen(k, 4 << 20, 70 + i) for i, k in enumerate(("silesia", "rand", "records", "text"))])
    n = base.size
    d_s = ctx.alloc(n); d_s.upload(base)
    d_d = ctx.alloc(n + 256 * 64 + 64)
    total, lens = ctx.lz4_compress_frames(d_s, n, d_d, 65536)
    comp = d_d.download(total).tobytes()
    d_s.free(); d_d.free()
    bodies, pos = [], 0
    for ln in lens:
        fr = comp[pos:pos + int(ln)]; pos += int(ln)
        (bl, _end) = W.blocks_of(fr)
        assert len(bl) == 1
        w, o, l = bl[0]
        bodies.append((fr[o:o + l], bool(w >> 31)))
    assert len(bodies) == 256
    return base.tobytes(), bodies


@pytest.mark.parametrize("bsum,csum,csize", [(1, 1, 1), (0, 1, 0), (1, 0, 1), (0, 0, 0)])
def test_a_16_mib_frame_of_256_blocks(ctx, blocks_16mib, bsum, csum, csize):
    src, bodies = blocks_16mib
    fr = W.frame(bodies, src, block_id=4, block_checksum=bool(bsum), content_checksum=bool(csum), content_size=len(src) if csize else None)
    bl, _ = W.blocks_of(fr)
    assert len(bl) == 256
    for route in ("blocks", "wave"):
        res, outs = decode(ctx, [fr], [len(src)], route, phase=3)
        assert res[0]["status"] == 0 and res[0]["in_used"] == len(fr) and res[0]["out_len"] == len(src), (route, res[0])
        assert outs[0] == src, route
    # one bit of block 200's body, and one of its checksum
    _, o, l = bl[200]
    damaged = [o + l // 2] + ([o + l + 1] if bsum else [])
    for at in damaged:
        bad = bytearray(fr); bad[at] ^= 0x10
        verdict = {}
        for route in ("blocks", "wave"):
            res, outs = decode(ctx, [bytes(bad)], [len(src)], route, phase=3)
            verdict[route] = int(res[0]["status"])
            if bsum or csum:
                assert res[0]["status"] != 0, (route, at)
            else:                                                   # nothing in such a frame catches a flipped literal
                assert res[0]["status"] != 0 or outs[0] != src, (route, at)
        assert (verdict["blocks"] == 0) == (verdict["wave"] == 0), verdict


def test_route_wave_and_auto_agree_without_candidates(ctx):
    parts = [datagen.gen_bytes("silesia", 50000 + 321 * i, 90 + i) for i in range(6)]
    frames = []
    for p in parts:
        d_s = ctx.alloc(len(p)); d_s.upload(p)
        d_d = ctx.alloc(len(p) + 128)
        total, _ = ctx.lz4_compress_frames(d_s, len(p), d_d, 65536)
        frames.append(d_d.download(total).tobytes())
        d_s.free(); d_d.free()
    a, oa = decode(ctx, frames, [len(p) for p in parts], "auto", phase=13)
    b, ob = decode(ctx, frames, [len(p) for p in parts], "wave", phase=13)
    assert (a == b).all() and oa == ob == parts and (a["status"] == 0).all()
