"""The LZ4 frame decoders (qatzip_amd/csrc/qzk_lz4.h) and the copy engine they share with inflate (qzk_lz_batch.h) sequence by
sequence on the CPU SIMT emulator: the matrix of tests/lz4_blocks_cases.py - blocks built so that a token, a ring position,
a batch boundary or a kind of copy is met on purpose - on the one-wave route and a wave per block, against the builder's
byte-by-byte model and what liblz4 1.9.3 answered (tests/golden/lz4_sequences/index.json, made by
tests/golden/gen_lz4_sequences.py).  The -m gpu twin is tests/test_gpu_lz4_sequences.py."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lz4_blocks_cases as K
import refcalls

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

with open(os.path.join(HERE, "golden", "lz4_sequences", "index.json")) as f:
    INDEX = {c["name"]: c for c in json.load(f)["cases"]}
CASES = K.cases()

SEG_DT = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("in_len", "<u4"), ("out_cap", "<u4")])
RES_DT = np.dtype([("status", "<i4"), ("in_used", "<u4"), ("out_len", "<u4"), ("pad", "<u4")])
ROUTES = {"auto": 0, "wave": 1, "blocks": 2}
GUARD = 64
# (wrapping, route): every frame on the kernel it is built for, and the blocks-route frames on the one-wave kernel as well
RUNS = (("wave", "wave"), ("blocks", "blocks"), ("blocks", "wave"), ("wave", "auto"), ("blocks", "auto"))


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


def decode(S, frames, caps, route, phase=K.PHASE, per_block=False):
    """the frames as the segments of ONE call, every output `phase` bytes off a 16-byte boundary and GUARD bytes of 0xA5
    behind every out_cap -> ([(status, in_used, out_len, output bytes or None)], block waves); the guards are checked here.
    per_block: every frame goes a wave per block, where a frame that does not fit is refused before a byte of it is written"""
    comp = np.frombuffer(b"".join(frames) + bytes(64), np.uint8).copy()
    segs = np.zeros(len(frames), SEG_DT)
    io, oo = 0, phase
    for i, (fr, cap) in enumerate(zip(frames, caps)):
        segs[i] = (io, oo, len(fr), cap)
        io += len(fr); oo += (cap + GUARD + 15) & ~15               # (every output at the same phase)
    out = np.full(oo + 64, 0xA5, np.uint8)
    res = np.zeros(len(frames), RES_DT)
    bw = C.c_uint32(0)
    assert S.sim_lz4_frames(comp.ctypes.data, out.ctypes.data, segs.ctypes.data, len(frames), ROUTES[route], res.ctypes.data, C.byref(bw)) == 0
    assert (out[:phase] == 0xA5).all()
    got = []
    for i in range(len(frames)):
        o, cap = int(segs[i]["out_off"]), int(segs[i]["out_cap"])
        end = int(segs[i + 1]["out_off"]) if i + 1 < len(frames) else out.size
        assert (out[o + cap:end] == 0xA5).all(), ("a store beyond out_cap", i, route)
        st = int(res[i]["status"])
        if st == -2 and per_block:
            assert (out[o:o + cap] == 0xA5).all(), ("output of a frame that does not fit", i)
        got.append((st, int(res[i]["in_used"]), int(res[i]["out_len"]), out[o:o + int(res[i]["out_len"])].tobytes() if st == 0 else None))
    return got, bw.value


@pytest.fixture(scope="module")
def frames():
    """{(case name, wrapping): frame}, built once"""
    return {(c.name, w): c.frame(w) for c in CASES for w in c.wrappings()}


@pytest.fixture(scope="module")
def decoded(sim, frames):
    """every run of RUNS, one call each: {(wrapping, route): ({case name: result}, block waves)}"""
    out = {}
    for w, route in RUNS:
        cs = [c for c in CASES if w in c.wrappings()]
        got, bw = decode(sim, [frames[c.name, w] for c in cs], [c.cap(w) for c in cs], route, per_block=w == "blocks" and route != "wave")
        out[w, route] = ({c.name: g for c, g in zip(cs, got)}, bw)
    return out


def test_the_builders_frames_are_the_ones_liblz4_judged(frames):
    assert [c.name for c in CASES] == list(INDEX)
    said, said_strict = set(), set()
    for c in CASES:
        rec = INDEX[c.name]
        assert rec["class"] == c.cls and c.cls in K.CLASSES, c.name
        assert [w for w in ("wave", "blocks") if w in rec] == list(c.wrappings()), c.name
        for w in c.wrappings():
            fr, r = frames[c.name, w], rec[w]
            assert len(fr) == r["len"] and _sha(fr) == r["sha"] and c.cap(w) == r["cap"], (c.name, w)
            said.add(r["liblz4"])
            if c.cls == K.STRICT:
                said_strict.add(r["liblz4"])
                if r["liblz4"] == "OK":                             # the model is liblz4's output
                    assert len(c.content(w)) == r["out_len"] and _sha(c.content(w)) == r["out_sha"], (c.name, w)
                if c.model is not None and c.cap_delta >= 0:        # nothing valid is left out of the parity
                    assert r["liblz4"] == "OK", (c.name, w)
    assert said == said_strict == {"OK", "ERROR_decompressionFailed", "ERROR_GENERIC", "incomplete"}
    exempt = [c for c in CASES if c.cls != K.STRICT]
    assert 5 * len(exempt) < len(CASES)
    assert {c.cls for c in exempt} == {K.LENIENT, K.OFFSET0}
    assert sorted(c.path for c in K.representatives()) == ["batch", "direct_lit", "direct_match", "stored"]


def test_the_builders_plan_of_the_batches():
    """the second-batch cases rest on K.batches(): its view of a block that other tests pin to the decoder's"""
    b = K.Block(1).seq(900, 300, K.RB_LIM - 12 - 900).seq(10, 19 + 25, 40).end()
    assert K.batches(b.records) == [(0, 1, 0, 0), (1, 2, 3060, 3060 - 9)]
    assert K.nmem_of(b.records, 1) == 25
    b = K.Block(1).seq(24, 7, 6).seq(1300, 11, 7).end()
    assert [x[1] for x in K.batches(b.records)] == [1, 0, 1]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_case_on_every_route(decoded, frames, c):
    verdicts = set()
    for w, route in RUNS:
        if w not in c.wrappings():
            continue
        st, used, olen, out = decoded[w, route][0][c.name]
        K.check(c, w, INDEX[c.name][w], frames[c.name, w], st, used, olen, out, (w, route))
        verdicts.add(st)
    assert len(verdicts) == 1, (c.name, verdicts)                   # the verdict does not depend on the route


def test_block_route_cases_took_block_waves(decoded):
    indep = [c for c in CASES if c.independent]
    for key in (("blocks", "blocks"), ("blocks", "auto")):
        assert decoded[key][1] == sum(2 + len(c.pre) for c in indep) > 0, key
    # frames of two independent blocks above the candidate length among the small ones: the history cases
    assert decoded["wave", "auto"][1] == sum(1 + len(c.pre) for c in indep if len(c.frame("wave")) > K.CAND) > 0
    for key in (("wave", "wave"), ("blocks", "wave")):
        assert decoded[key][1] == 0


@pytest.mark.parametrize("phase", range(16))
def test_every_output_phase(sim, frames, phase):
    """one case per path with its output at every phase of a 16-byte row: the first row, `hd`, the masked flush"""
    reps = K.representatives()
    for w, route in RUNS[:3]:
        got, _ = decode(sim, [frames[c.name, w] for c in reps], [c.cap(w) for c in reps], route, phase=phase, per_block=w == "blocks" and route != "wave")
        for c, (st, used, olen, out) in zip(reps, got):
            K.check(c, w, INDEX[c.name][w], frames[c.name, w], st, used, olen, out, (w, route, phase))


@pytest.mark.skipif(not refcalls.lz4_pinned(), reason="needs liblz4 1.9.3")
def test_random_blocks_against_liblz4(sim):
    """300 blocks of the builder's random mode (valid, obeying the end rules): liblz4, the model and both routes agree"""
    from gen_lz4_blocks import lz4f_decompress
    cs = K.random_cases(300, 20241)
    for w, route in RUNS[:2]:
        frs = [c.frame(w) for c in cs]
        if w == "wave":
            for c, fr in zip(cs, frs):
                v, back = lz4f_decompress(fr, c.cap(w))
                assert v == "OK" and back == c.model, c.name
        got, bw = decode(sim, frs, [c.cap(w) for c in cs], route, phase=11, per_block=route == "blocks")
        assert bw == (2 * len(cs) if route == "blocks" else 0)
        for c, fr, (st, used, olen, out) in zip(cs, frs, got):
            assert st == 0 and used == len(fr) and out == c.content(w), (c.name, route, st)
