"""The inflate kernels on hand-built deflate edge cases (tests/deflate_writer.py), through the SIMT emulator: the
wave-per-segment kernel, the serial lane phase A + phase B, and the speculative K-lane phase A for K = 4, 8, 16, 32.
Each case alone and embedded after 20 KB of ordinary content at several bit phases (there, lanes other than lane 0 of
the K-lane kernel meet the edge).  zlib is the reference: a valid case decodes to zlib's bytes with zlib's in_used, an
invalid one (zlib rejects it) ends in an error with nothing written past the segment's output."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deflate_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)
SEG_DT = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("in_len", "<u4"), ("out_cap", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
RES_DT = np.dtype([("status", "<i4"), ("in_used", "<u4"), ("out_len", "<u4"), ("nblocks", "<u4")])
PHASES = (1, 4, 7)
INVALID_CAP = 1 << 17


@pytest.fixture(scope="module")
def decoders():
    so = os.path.join(SIMDIR, "libqzsim.so")
    deps = [os.path.join(SIMDIR, f) for f in ("sim_driver.cpp", "hipsim.h")]
    csrc = os.path.join(ROOT, "qatzip_amd", "csrc")
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-I", SIMDIR,
                               "-Wno-unused-function", "-o", so, os.path.join(SIMDIR, "sim_driver.cpp")])
    S = C.CDLL(so)
    for f in (S.sim_inflate, S.sim_inflate_lane):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    S.sim_inflate_spec.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
    out = [("wave", S.sim_inflate), ("lane", S.sim_inflate_lane)]
    for K in (4, 8, 16, 32):
        out.append(("k%d" % K, lambda a, b, c, d, e, K=K: S.sim_inflate_spec(a, b, c, d, e, K)))
    return out


def _run(fn, comp, cap):
    """one segment: the whole stream, out_cap = cap, the compressed length as the hint; -> (bytes, result, canary)"""
    cbuf = np.frombuffer(comp + b"\0" * 64, np.uint8).copy()
    obuf = np.full(cap + 64, 0xAA, np.uint8)
    sa = np.array([(0, 0, len(comp), cap, 0, len(comp))], dtype=SEG_DT)
    res = np.zeros(1, RES_DT)
    fn(cbuf.ctypes.data, obuf.ctypes.data, sa.ctypes.data, res.ctypes.data, 1)
    return bytes(obuf[:cap]), res[0], bytes(obuf[cap:])


def _streams(name, fn, valid):
    yield "alone", W.build_case(fn)
    if valid or name not in W.LONE_ONLY:
        for ph in (PHASES if valid else PHASES[1:2]):
            yield "phase%d" % ph, W.build_case(fn, 20480, ph)


@pytest.mark.parametrize("name", sorted(W.VALID))
def test_valid_case_decodes_to_zlibs_bytes(decoders, name):
    for where, comp in _streams(name, W.VALID[name], True):
        ok, want, in_used = W.reference(comp)
        assert ok, (name, where, "zlib rejects the writer's stream")
        for dec, fn in decoders:
            got, r, tail = _run(fn, comp, len(want))
            assert tail == b"\xaa" * 64, (name, where, dec)
            assert int(r["status"]) == 0, (name, where, dec, int(r["status"]))
            assert int(r["out_len"]) == len(want) and got == want, (name, where, dec)
            assert int(r["in_used"]) == in_used, (name, where, dec, int(r["in_used"]), in_used)


@pytest.mark.parametrize("name", sorted(W.INVALID))
def test_invalid_case_is_an_error(decoders, name):
    for where, comp in _streams(name, W.INVALID[name], False):
        ok, _, _ = W.reference(comp)
        assert not ok, (name, where, "zlib accepts the case: the corpus has drifted from the reference")
        for dec, fn in decoders:
            got, r, tail = _run(fn, comp, INVALID_CAP)
            assert tail == b"\xaa" * 64, (name, where, dec)
            assert int(r["status"]) < 0, (name, where, dec, int(r["status"]), int(r["out_len"]))


def test_corpus_size():
    """the corpus covers what it claims: every listed construct, each checked against zlib by the tests above"""
    assert len(W.VALID) >= 18 and len(W.INVALID) >= 21
