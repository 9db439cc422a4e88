"""The LZ4-HC kernels (qatzip_amd/csrc/qzk_lz4hc.h: chains, parse, finish) on the CPU SIMT emulator against what liblz4 1.9.3
wrote (tests/golden/lz4hc, made by tests/golden/gen_lz4hc.py) and, where that library is installed, against the library
itself on random shapes.  The -m gpu twin is tests/test_gpu_lz4hc.py.

What the emulator runs is fixed: every index case with n <= 131073 at every level 3-8, the larger ones (200777, 300000) at
levels 3 and 8; every block-store edge case; every whole-frame file.  The 1 MiB cases are left to the GPU test, which runs
every case: with them the emulator run alone took seven minutes on eight cores.  The cases are spread over worker processes (the
emulator keeps its fibers in globals: one launch at a time per process)."""
import ctypes as C
import hashlib
import json
import multiprocessing
import os
import random
import struct
import subprocess
import sys

import pytest

import datagen
import refcalls

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "lz4hc")
sys.path.insert(0, os.path.join(HERE, "golden"))

with open(os.path.join(GOLD, "index.json")) as f:
    INDEX = json.load(f)

_S = None


def _load(so):
    global _S
    if _S is None:
        S = C.CDLL(so)
        S.sim_lz4hc.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                C.POINTER(C.c_uint64), C.c_void_p]
        S.sim_lz4hc_block.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p]
        S.sim_lz4hc_block.restype = C.c_uint32
        S.sim_lz4hc_stride.restype = C.c_uint32
        _S = S
    return _S


def sim_frames(so, src, level, frame_sz=None, hw=0, batch=0):
    S = _load(so)
    n = len(src)
    fs = frame_sz or max(n, 1)
    nb = n // 65536 + n // fs + 2
    cap = n + 64 + 32 * nb
    out = C.create_string_buffer(cap); ol = C.c_uint64(0)
    lens = (C.c_uint32 * nb)()
    rc = S.sim_lz4hc(src, n, fs, level, hw, batch, out, cap, C.byref(ol), lens)
    assert rc == 0, rc
    return out.raw[:ol.value]


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def words_of(frame):
    pos = 15 if frame[4] & 8 else 7
    out = []
    while True:
        w = struct.unpack_from("<I", frame, pos)[0]
        pos += 4
        if w == 0:
            return out
        out.append(w)
        pos += w & 0x7fffffff


def _run_case(arg):
    """one golden case in a worker: None, or what went wrong"""
    so, what, c = arg
    if what == "edge":
        import gen_lz4hc
        src = gen_lz4hc.barely(c["seed"], c["n"])
    else:
        src = datagen.gen_bytes(c["kind"], c["n"], c["seed"])
    if _sha(src) != c["in_sha"]:
        return ("input differs from the one the fixture was made of", what, c.get("kind"), c["n"], c["level"])
    got = sim_frames(so, src, c["level"], batch=c.get("batch", 0))
    if len(got) != c["out_len"] or _sha(got) != c["out_sha"]:
        return ("frame differs", what, c.get("kind"), c["n"], c["level"], len(got), c["out_len"])
    if "words" in c and words_of(got) != c["words"]:
        return ("block words differ", what, c.get("kind"), c["n"], c["level"])
    if "file" in c:
        with open(os.path.join(GOLD, c["file"]), "rb") as f:
            if got != f.read():
                return ("file differs", c["file"])
    return None


@pytest.fixture(scope="module")
def simso():
    so = os.path.join(SIMDIR, "libqzsim_lz4hc.so")
    deps = [os.path.join(SIMDIR, f) for f in ("sim_lz4hc.cpp", "hipsim.h")]
    csrc = os.path.join(ROOT, "qatzip_amd", "csrc")
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-I", SIMDIR, "-Wno-unused-function",
                               "-o", so, os.path.join(SIMDIR, "sim_lz4hc.cpp")])
    return so


def _pool():
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    return multiprocessing.get_context("fork").Pool(max(1, min(8, cpus)))


def _selected_cases():
    return [c for c in INDEX["cases"] if c["n"] <= 131073 or (c["level"] in (3, 8) and c["n"] < (1 << 20))]


def test_the_rule_selects_what_it_says():
    sel = _selected_cases()
    assert len(INDEX["cases"]) == 8 * 14 * 6
    assert len(sel) == 8 * (11 * 6 + 2 * 2)
    assert {c["level"] for c in sel} == {3, 4, 5, 6, 7, 8} and {c["kind"] for c in sel} == set(datagen.KINDS)


def test_index_cases_match_liblz4(simso):
    """every case the rule names, largest first so that the workers end together"""
    work = [(simso, "case", c) for c in sorted(_selected_cases(), key=lambda c: -c["n"])]
    with _pool() as p:
        bad = [r for r in p.imap_unordered(_run_case, work, chunksize=1) if r]
    assert not bad, bad[:10]


def test_block_store_edges_and_whole_frames(simso):
    """blocks that end within a byte or three of the n - 1 a frame allows them, on either side; and the committed frames
    byte for byte, once in one round and once in rounds of two blocks"""
    outcomes = {(e["n"], e["level"], e["outcome"]) for e in INDEX["edge"]}
    assert {o for _, _, o in outcomes} == {"over", "under"}
    for e in INDEX["edge"]:
        assert bool(e["words"][-1] & 0x80000000) == (e["outcome"] == "over") and abs(e["margin"]) <= 5, e
    work = [(simso, "edge", e) for e in INDEX["edge"]] + [(simso, "file", f) for f in INDEX["files"]] + \
           [(simso, "file", dict(f, batch=2)) for f in INDEX["files"] if f["n"] > 131072]
    with _pool() as p:
        bad = [r for r in p.imap_unordered(_run_case, work, chunksize=1) if r]
    assert not bad, bad


def test_blocks_of_a_linked_frame_parse_alone(simso):
    """the independence the design rests on, tested as such: block k of a multi-block input, its chains and its parse made
    by a launch that sees nothing of the other blocks' work, is the block liblz4 wrote at that place in the frame"""
    S = _load(simso)
    seen = 0
    for fr in INDEX["files"]:
        if (fr["kind"], fr["level"]) not in (("text", 8), ("silesia", 3), ("records", 8)) or fr["n"] <= 131072:
            continue
        src = datagen.gen_bytes(fr["kind"], fr["n"], fr["seed"])
        with open(os.path.join(GOLD, fr["file"]), "rb") as f:
            gold = f.read()
        pos = 15
        nb = (fr["n"] + 65535) // 65536
        for k in range(nb):
            w = struct.unpack_from("<I", gold, pos)[0]
            blk = gold[pos:pos + 4 + (w & 0x7fffffff)]
            pos += len(blk)
            if k == 0:
                continue                                            # (a frame's first block has nothing in front of it)
            slot = C.create_string_buffer(S.sim_lz4hc_stride())
            ln = S.sim_lz4hc_block(src, fr["n"], fr["n"], fr["level"], k, slot)
            got = slot.raw[:ln - (8 if k == nb - 1 else 0)]
            assert got == blk, (fr["file"], k)
            seen += 1
    assert seen == 3 + 4 + 4


def test_hw_framing_chunks(simso):
    """the hardware path's framing on the emulator: a frame per chunk behind the FLG 0x4C header, linked above 64 KB"""
    hw = [h for h in INDEX["hw"] if (h["kind"], h["level"]) in (("records", 3), ("rand", 8))]
    assert len(hw) == 4
    for h in hw:
        src = datagen.gen_bytes(h["kind"], h["n"], h["seed"])
        got = sim_frames(simso, src, h["level"], frame_sz=h["hw_buff_sz"], hw=1)
        pos = 0
        for i, ch in enumerate(h["chunks"]):
            piece = src[i * h["hw_buff_sz"]:(i + 1) * h["hw_buff_sz"]]
            assert got[pos:pos + 6] == bytes([0x04, 0x22, 0x4D, 0x18, 0x4C, 0x40]), (h["kind"], h["hw_buff_sz"], i)
            assert got[pos + 6:pos + 14] == len(piece).to_bytes(8, "little")
            body = got[pos + 15:pos + 15 + ch["len"]]
            assert _sha(body) == ch["sha"], (h["kind"], h["hw_buff_sz"], h["level"], i)
            pos += 15 + ch["len"]
        assert pos == len(got)


def test_levels_outside_3_to_8_are_not_run(simso):
    S = _load(simso)
    out = C.create_string_buffer(256); ol = C.c_uint64(0)
    for lvl in (0, 1, 2, 9, 10, 12):
        assert S.sim_lz4hc(b"x" * 20, 20, 20, lvl, 0, 0, out, 256, C.byref(ol), None) == -2


@pytest.mark.skipif(not refcalls.lz4_pinned(), reason="liblz4 1.9.3 is not installed here")
def test_random_shapes_against_the_library(simso):
    rng = random.Random(20240607)
    for i in range(20):
        kind = rng.choice(datagen.KINDS)
        n = rng.choice([rng.randrange(0, 200), rng.randrange(200, 9000), rng.randrange(9000, 70000), rng.randrange(65000, 150000)])
        if kind == "lzmix":
            n = min(n, 70000)
        src = datagen.gen_bytes(kind, n, 900 + i)
        if n > 64 and rng.random() < 0.4:
            cut = rng.randrange(1, n); src = (src[cut:] + src[:cut] + src)[:n]
        lvl = rng.randrange(3, 9)
        batch = rng.choice([0, 1, 2])
        assert sim_frames(simso, src, lvl, batch=batch) == refcalls.lz4f_compress_frame(src, lvl), (kind, n, 900 + i, lvl, batch)
