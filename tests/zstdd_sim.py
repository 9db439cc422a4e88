"""The zstd decode kernels (qatzip_amd/csrc/qzk_zstdd.h) on the CPU SIMT emulator: used by tests/test_sim_zstdd.py and
tests/golden/gen_zstd_dec.py; the index of tests/golden/zstd_dec/ for the GPU tests as well."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)
SO = os.path.join(SIMDIR, "libqzsim_zstdd.so")
GOLDEN = os.path.join(HERE, "golden", "zstd_dec")
EDATA, EOUT, ETRUNC, ECKSUM, EUNSUP = -1, -2, -3, -4, -5

SEG = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("in_len", "<u4"), ("out_cap", "<u4")])
RES = np.dtype([("status", "<i4"), ("in_used", "<u4"), ("out_len", "<u4"), ("pad", "<u4")])

_S = None


def _deps():
    deps = [os.path.join(SIMDIR, f) for f in ("sim_zstdd.cpp", "hipsim.h")]
    csrc = os.path.join(ROOT, "qatzip_amd", "csrc")
    return deps + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]


def build_so():
    """g++ build of tests/sim/sim_zstdd.cpp, redone when a source is newer"""
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in _deps()):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-I", SIMDIR, "-Wno-unused-function",
                               "-o", SO, os.path.join(SIMDIR, "sim_zstdd.cpp")])
    return SO


def _load():
    global _S
    if _S is None:
        S = C.CDLL(build_so())
        S.sim_zstdd_frames.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                       C.POINTER(C.c_uint32)]
        S.sim_zstdd_extent.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint32)]
        S.sim_zstdd_extent.restype = C.c_int64
        S.sim_zstdd_group.restype = C.c_uint32
        _S = S
    return _S


def group():
    """frames per wave of stage E"""
    return _load().sim_zstdd_group()


def extent(buf):
    """qzd_zd_frame_walk -> (length or < 0, content, has_content, bound, blocks)"""
    content, has, bound, nb = C.c_uint64(0), C.c_int(0), C.c_uint64(0), C.c_uint32(0)
    r = _load().sim_zstdd_extent(bytes(buf), len(buf), C.byref(content), C.byref(has), C.byref(bound), C.byref(nb))
    return r, content.value, bool(has.value), bound.value, nb.value


def decode(comp, segs, out_size, scratch_cap=0):
    """-> (guard rc, results, the output image, rounds)"""
    S = _load()
    segs = np.ascontiguousarray(segs, dtype=SEG)
    res = np.zeros(max(len(segs), 1), dtype=RES)
    out = C.create_string_buffer(out_size + 1)
    rounds = C.c_uint32(0)
    rc = S.sim_zstdd_frames(bytes(comp), segs.ctypes.data, len(segs), out, out_size, res.ctypes.data, scratch_cap, C.byref(rounds))
    return rc, res[:len(segs)], out.raw[:out_size], rounds.value


def layout(frames, caps, gap=0):
    """the frames back to back, their outputs `gap` bytes apart (0: back to back, sharing 16-byte rows) -> (comp, segs,
    out_size)"""
    segs = np.zeros(len(frames), dtype=SEG)
    ti, to = 0, gap
    for i, (f, cap) in enumerate(zip(frames, caps)):
        segs[i] = (ti, to, len(f), cap)
        ti += len(f)
        to += cap + gap
    return b"".join(frames), segs, to + 16


def decode_frames(frames, caps, gap=0, scratch_cap=0):
    """-> ([(status, in_used, out_len)], [each frame's output]); asserts the guards"""
    comp, segs, out_size = layout(frames, caps, gap)
    rc, res, out, _ = decode(comp, segs, out_size, scratch_cap)
    assert rc == 0, "guard bytes were written (rc %d)" % rc
    outs = [out[int(s["out_off"]):int(s["out_off"]) + int(r["out_len"])] for s, r in zip(segs, res)]
    return [(int(r["status"]), int(r["in_used"]), int(r["out_len"])) for r in res], outs


def index():
    with open(os.path.join(GOLDEN, "index.json")) as f:
        return json.load(f)


def frame_bytes(entry):
    with open(os.path.join(GOLDEN, entry["file"]), "rb") as f:
        return f.read()
