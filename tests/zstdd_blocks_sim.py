"""The block route of the zstd decoder (qatzip_amd/csrc/qzk_zstdd_blocks.h) on the CPU SIMT emulator: used by
tests/test_sim_zstdd_blocks.py and tests/golden/gen_zstd_dec_blocks.py; the index of tests/golden/zstd_dec_blocks/ for the GPU
tests as well."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import zstdd_sim as D

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)
SRC = os.path.join(SIMDIR, "sim_zstdd_blocks.cpp")
SO = os.path.join(SIMDIR, "libqzsim_zstdd_blocks.so")
GOLDEN = os.path.join(HERE, "golden", "zstd_dec_blocks")
EHINT = -6
ROUTES = {"auto": 0, "frame": 1, "blocks": 2}

_S = None


def _deps():
    csrc = os.path.join(ROOT, "qatzip_amd", "csrc")
    return [SRC, os.path.join(SIMDIR, "hipsim.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]


def build_so():
    """g++ build of tests/sim/sim_zstdd_blocks.cpp, redone when a source is newer"""
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in _deps()):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-I", SIMDIR, "-Wno-unused-function", "-o", SO, SRC])
    return SO


def _load():
    global _S
    if _S is None:
        S = C.CDLL(build_so())
        u32p = C.POINTER(C.c_uint32)
        S.sim_zstddb_frames_fb.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_uint64, u32p, u32p, u32p, C.c_void_p]
        S.sim_zstddb_count.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p]
        S.sim_zstddb_count.restype = None
        for f in (S.sim_zstddb_group, S.sim_zstddb_min, S.sim_zstddb_desc_size):
            f.restype = C.c_uint32
        _S = S
    return _S


def group():
    return _load().sim_zstddb_group()


def blocks_min():
    return _load().sim_zstddb_min()


def decode(comp, segs, out_size, nblocks=None, route="blocks", scratch_cap=0):
    """-> (guard rc, results, the output image, {rounds, routed, launches, fail_blk: per segment the earliest refused block of
    a routed frame, -1 where there is none})"""
    S = _load()
    segs = np.ascontiguousarray(segs, dtype=D.SEG)
    res = np.zeros(max(len(segs), 1), dtype=D.RES)
    out = C.create_string_buffer(out_size + 1)
    nb = None if nblocks is None else np.ascontiguousarray(nblocks, dtype=np.uint32)
    assert nb is None or len(nb) == len(segs)
    rounds, routed, launches = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    fail = np.zeros(max(len(segs), 1), dtype=np.int32)
    rc = S.sim_zstddb_frames_fb(bytes(comp), segs.ctypes.data, len(segs), out, out_size, res.ctypes.data, None if nb is None else nb.ctypes.data,
                                ROUTES[route], scratch_cap, C.byref(rounds), C.byref(routed), C.byref(launches), fail.ctypes.data)
    return rc, res[:len(segs)], out.raw[:out_size], {"rounds": rounds.value, "routed": routed.value, "launches": launches.value,
                                                     "fail_blk": [int(x) for x in fail[:len(segs)]]}


def decode_frames(frames, caps, nblocks=None, route="blocks", gap=0, scratch_cap=0, info=None):
    """-> ([(status, in_used, out_len)], [each frame's output]); asserts the guards.  nblocks None: every frame's count from
    the host's walk (0 where it fails)"""
    comp, segs, out_size = D.layout(frames, caps, gap)
    if nblocks is None:
        nblocks = [walk_count(f) for f in frames]
    rc, res, out, st = decode(comp, segs, out_size, nblocks, route, scratch_cap)
    assert rc == 0, "guard bytes were written (rc %d)" % rc
    if info is not None:
        info.update(st)
    outs = [out[int(s["out_off"]):int(s["out_off"]) + int(r["out_len"])] for s, r in zip(segs, res)]
    return [(int(r["status"]), int(r["in_used"]), int(r["out_len"])) for r in res], outs


def walk_count(frame):
    """the host's walk (qzd_zd_frame_walk): the frame's blocks, 0 where the walk fails"""
    ext, _, _, _, nb = D.extent(frame)
    return nb if ext > 0 else 0


def count_blocks(frames):
    """the device's walk (qzd_zstd_count_blocks)"""
    comp, segs, _ = D.layout(frames, [0] * len(frames))
    nb = np.zeros(max(len(frames), 1), dtype=np.uint32)
    _load().sim_zstddb_count(bytes(comp), segs.ctypes.data, len(frames), nb.ctypes.data)
    return [int(x) for x in nb[:len(frames)]]


def index():
    with open(os.path.join(GOLDEN, "index.json")) as f:
        return json.load(f)


def frame_bytes(entry):
    with open(os.path.join(GOLDEN, entry["file"]), "rb") as f:
        return f.read()
