"""The LZ4 frame decoders (qatzip_amd/csrc/qzk_lz4.h: the one-wave kernel and the plan / size / scan / block / finish kernels
that give every block of an independent-block frame a wave of its own) on the CPU SIMT emulator, on both routes, against
tests/golden/lz4_blocks: frames liblz4 1.9.3 wrote and hand-built ones with what its LZ4F_decompress answered
(tests/golden/gen_lz4_blocks.py).  The -m gpu twin is tests/test_gpu_lz4_blocks.py."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "lz4_blocks")
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_lz4_blocks  # noqa: E402

with open(os.path.join(GOLD, "index.json")) as f:
    INDEX = json.load(f)

SEG_DT = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("in_len", "<u4"), ("out_cap", "<u4")])
RES_DT = np.dtype([("status", "<i4"), ("in_used", "<u4"), ("out_len", "<u4"), ("pad", "<u4")])
ROUTES = {"auto": 0, "wave": 1, "blocks": 2}
GUARD = 64


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIMDIR, "libqzsim_lz4blocks.so")
    deps = [os.path.join(SIMDIR, f) for f in ("sim_lz4blocks.cpp", "hipsim.h")]
    csrc = os.path.join(ROOT, "qatzip_amd", "csrc")
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-I", SIMDIR, "-Wno-unused-function",
                               "-o", so, os.path.join(SIMDIR, "sim_lz4blocks.cpp")])
    S = C.CDLL(so)
    S.sim_lz4_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_uint32)]
    return S


@pytest.fixture(scope="module")
def verdict_frames():
    """the writer's frames, once: name -> (frame, cap_short)"""
    return {name: (fr, short) for name, fr, short in gen_lz4_blocks.verdict_frames()}


def decode(S, frames, caps, route, phase=5):
    """the frames as the segments of ONE call, outputs `phase` bytes off a 16-byte boundary and GUARD bytes of 0xA5 behind
    every out_cap -> (results, [output bytes of each segment], block waves); the guards are checked here"""
    comp = np.frombuffer(b"".join(frames), np.uint8).copy()
    comp = np.concatenate([comp, np.zeros(64, np.uint8)])
    segs = np.zeros(len(frames), SEG_DT)
    io, oo = 0, phase
    for i, (fr, cap) in enumerate(zip(frames, caps)):
        segs[i] = (io, oo, len(fr), cap)
        io += len(fr); oo += cap + GUARD + 3
    out = np.full(oo + 64, 0xA5, np.uint8)
    res = np.zeros(len(frames), RES_DT)
    bw = C.c_uint32(0)
    assert S.sim_lz4_frames(comp.ctypes.data, out.ctypes.data, segs.ctypes.data, len(frames), ROUTES[route], res.ctypes.data, C.byref(bw)) == 0
    assert (out[:phase] == 0xA5).all()
    outs = []
    for i in range(len(frames)):
        o, cap = int(segs[i]["out_off"]), int(segs[i]["out_cap"])
        assert (out[o + cap:o + cap + GUARD + 3] == 0xA5).all(), ("a store beyond out_cap", i, route)
        if res[i]["status"] == -2:
            assert (out[o:o + cap] == 0xA5).all() or route == "wave", ("output of a frame that does not fit", i)
        outs.append(out[o:o + int(res[i]["out_len"])].tobytes() if res[i]["status"] == 0 else None)
    return res, outs, bw.value


def test_the_writers_frames_are_the_ones_liblz4_judged(verdict_frames):
    assert [v["name"] for v in INDEX["verdicts"]] == list(verdict_frames)
    for v in INDEX["verdicts"]:
        fr, short = verdict_frames[v["name"]]
        assert len(fr) == v["len"] and _sha(fr) == v["sha"] and short == v["cap_short"], v["name"]
    said = {v["liblz4"] for v in INDEX["verdicts"]}
    assert said == {"OK", "ERROR_blockChecksum_invalid", "ERROR_GENERIC", "ERROR_maxBlockSize_invalid"}


@pytest.mark.parametrize("v", INDEX["verdicts"], ids=lambda v: v["name"])
def test_verdicts_on_both_routes(sim, verdict_frames, v):
    fr, short = verdict_frames[v["name"]]
    ok = v["liblz4"] == "OK"
    cap = v["out_len"] - short if ok else 80000
    got = {}
    for route in ("blocks", "wave", "auto"):
        res, outs, bw = decode(sim, [fr], [cap], route)
        r = res[0]
        if ok and not short:
            assert r["status"] == 0 and r["in_used"] == len(fr) and r["out_len"] == v["out_len"], (route, r)
            assert _sha(outs[0]) == v["out_sha"], route
        else:
            assert r["status"] != 0, (route, r)
        got[route] = (int(r["status"]), outs[0])
        if route == "wave":
            assert bw == 0
        elif v["name"] in ("8000_stored_blocks", "cross_block_linked"):
            assert bw == 0                                          # more blocks than its share of the table; linked
        elif v["name"] not in ("block_above_bd_max", "end_mark_missing"):
            assert bw in (2, 3), (route, bw)                        # (those two end in the plan kernel)
    assert got["blocks"] == got["wave"] == got["auto"], v["name"]
    if short:
        assert got["blocks"][0] == -2


@pytest.mark.parametrize("f", [f for f in INDEX["files"] if f["n"] <= 300000], ids=lambda f: f["file"])
def test_liblz4_frames_on_both_routes(sim, f):
    with open(os.path.join(GOLD, f["file"]), "rb") as fh:
        fr = fh.read()
    assert _sha(fr) == f["out_sha"]
    src = datagen.gen_bytes(f["kind"], f["n"], f["seed"])
    assert _sha(src) == f["in_sha"]
    for route in ("blocks", "wave"):
        for cap in (f["n"], f["n"] + 1000):
            res, outs, bw = decode(sim, [fr], [cap], route, phase=11)
            assert res[0]["status"] == 0 and res[0]["in_used"] == len(fr) and res[0]["out_len"] == f["n"], (route, cap, res[0])
            assert outs[0] == src, (route, cap)
            assert bw == (f["blocks"] if route == "blocks" and len(fr) > 65571 else 0)


def test_mixed_segments_in_one_call(sim, verdict_frames):
    """small frames, block-route frames, a linked one, the many-block one and a damaged one side by side, every output at an
    odd address: each result is its own and no output disturbs its neighbour (decode() checks the guards)"""
    small = [datagen.gen_bytes("text", 3000 + 7 * i, 30 + i) for i in range(2)]
    import lz4_frame_writer as W
    frames = [W.frame([(W.literals_block(s), False)], s, content_checksum=True, content_size=len(s)) for s in small]
    names = ["three_blocks_cc", "cross_block_linked", "8000_stored_blocks", "three_blocks_nocc_badsum1", "dict_id"]
    frames += [verdict_frames[n][0] for n in names]
    by = {v["name"]: v for v in INDEX["verdicts"]}
    caps = [len(s) for s in small] + [by[n].get("out_len", 80001) for n in names]
    for route in ("auto", "wave"):
        res, outs, bw = decode(sim, frames, caps, route, phase=9)
        assert bw == (0 if route == "wave" else 3 + 3 + 2)
        for i, s in enumerate(small):
            assert res[i]["status"] == 0 and outs[i] == s
        for i, n in enumerate(names, len(small)):
            if by[n]["liblz4"] == "OK":
                assert res[i]["status"] == 0 and res[i]["in_used"] == len(frames[i]) and _sha(outs[i]) == by[n]["out_sha"], (route, n)
            else:
                assert res[i]["status"] == -1, (route, n)
