"""The deflate compressors on trap inputs (tests/deflate_traps.py) without a GPU: every trap is live in zlib's own output,
the goldens (tests/golden/traps.json) are libz's bytes, the oracle reproduces them, and so do the kernel bodies run on
the SIMT emulator (tests/sim/) - K1, K1 fused with K2, K1w and K1b at level 1, K1b at levels 2-3, the lazy kernels at
4-9, the coalesced launch at 1 / 3 / 6 - with the per-chunk CRC-32 of every run."""
import collections
import ctypes as C
import hashlib
import json
import os
import subprocess
import time
import zlib

import numpy as np
import pytest

import deflate_traps as T
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "traps.json")


def sha(b, n=24):
    return hashlib.sha256(b).hexdigest()[:n]


@pytest.fixture(scope="module")
def traps():
    t = time.time()
    cases = {c.name: c for c in T.all_cases()}
    with open(GOLDEN) as f:
        g = json.load(f)
    runs = {(r[0], r[1], r[2], r[3], r[4]): r for r in g["runs"]}
    print("\n%d trap cases, %d golden runs, built in %.1f s" % (len(cases), len(runs), time.time() - t))
    return cases, g, runs


def _golden_ok(run, out):
    return len(out) == run[5] and sha(out) == run[6] and (not run[7] or out.hex() == run[7])


def test_trap_inputs_are_the_recorded_ones(traps):
    cases, g, runs = traps
    assert set(cases) == set(g["cases"])
    for name, c in cases.items():
        assert [len(c.data), sha(c.data, 16)] == g["cases"][name], name
    assert {r[0] for r in runs.values()} == set(cases)


@pytest.mark.skipif(zlib.ZLIB_RUNTIME_VERSION != "1.2.11", reason="the liveness checks read libz 1.2.11's own decisions")
def test_every_trap_is_live(traps):
    """a case whose decision zlib's output does not show tests nothing: each one must show it, at each of its levels"""
    cases, _, _ = traps
    live, dead, tiny = collections.Counter(), [], []
    for c in cases.values():
        for lv in c.levels:
            z = T.zlib_parse(c.data, lv, c.hw)
            if c.family == "F7tiny":
                tiny.append(z)
                live[c.family] += 1
            elif c.check(z, lv):
                live[c.family] += 1
            else:
                dead.append((c.name, lv, c.aim))
    print("\nlive (case, level) pairs per family:", dict(sorted(live.items())))
    assert not dead, dead[:20]
    assert all(live[f] > 0 for f in T.FAMILIES), live
    assert T.tiny_types_ok(tiny), "the tiny inputs must show stored, fixed and dynamic blocks"


@pytest.mark.skipif(zlib.ZLIB_RUNTIME_VERSION != "1.2.11", reason="needs libz 1.2.11")
def test_goldens_regenerate_byte_identically():
    import refcalls as R
    if not R.libz_pinned():
        pytest.skip("needs libz.so.1 1.2.11")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_traps", os.path.join(HERE, "golden", "gen_traps.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(GOLDEN) as f:
        assert gen.build() == f.read()


def test_oracle_on_every_trap(traps):
    """the oracle most GPU tests compare with, pinned on the traps too"""
    cases, _, runs = traps
    for (name, fmt, lv, hw, last), r in runs.items():
        src = cases[name].data
        rc, _, out, _ = O.sw_compress(fmt, src, hw, lv, last=last, cap=len(src) * 9 // 8 + 8192)
        assert rc == 0 and _golden_ok(r, out), (name, fmt, lv, hw, last, len(out), r[5])


# ------------------------------------------------------------------------------------------------ the emulator
@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIMDIR, "libqzsim.so")
    deps = [os.path.join(SIMDIR, f) for f in ("sim_driver.cpp", "hipsim.h")]
    csrc = os.path.join(ROOT, "qatzip_amd", "csrc")
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-I", SIMDIR,
                               "-Wno-unused-function", "-o", so, os.path.join(SIMDIR, "sim_driver.cpp")])
    S = C.CDLL(so)
    a4 = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    for f in ("sim_deflate", "sim_deflate_fused", "sim_deflate_wide", "sim_deflate_lane"):
        getattr(S, f).argtypes = a4
    S.sim_deflate_level.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    S.sim_deflate_lazy.argtypes = S.sim_deflate_level.argtypes
    S.sim_deflate_ragged.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return S


def _run(S, fn, src, hw, last, level=None):
    n = len(src)
    nch = max(1, (n + hw - 1) // hw)
    cap = n * 9 // 8 + 4096 * (nch + 1)
    out = C.create_string_buffer(cap); ol = C.c_uint64(0); crcs = np.zeros(nch, np.uint32)
    if level is None:
        getattr(S, fn)(src, n, hw, last, out, C.byref(ol), crcs.ctypes.data)
    else:
        getattr(S, fn)(src, n, hw, last, level, out, C.byref(ol), crcs.ctypes.data)
    return out.raw[:ol.value], crcs


def _check_crcs(src, hw, crcs):
    for i in range(len(crcs) if src else 0):
        assert int(crcs[i]) == zlib.crc32(src[i * hw:(i + 1) * hw]) & 0xffffffff, i


def _select(runs, cases, level, fmt="RAW", max_len=None, hw_max=None):
    out = []
    for (name, f, lv, hw, last), r in sorted(runs.items()):
        if f != fmt or lv != level:
            continue
        n = len(cases[name].data)
        if (max_len and n > max_len) or (hw_max and hw > hw_max):
            continue
        out.append((name, hw, last, r))
    return out


@pytest.mark.parametrize("fn", ["sim_deflate_fused", "sim_deflate", "sim_deflate_lane", "sim_deflate_wide"])
def test_level1_kernels_on_traps(sim, traps, fn):
    """K1 fused with K2 (the product's shape) and K1 + K2 as launches of their own on every level-1 run, K1b likewise;
    K1w (chunks of at most 64 KiB) on every run of up to 40 000 bytes"""
    cases, _, runs = traps
    sel = _select(runs, cases, 1, hw_max=65536 if fn == "sim_deflate_wide" else None,
                  max_len=40000 if fn == "sim_deflate_wide" else None)
    t = time.time()
    for name, hw, last, r in sel:
        src = cases[name].data
        out, crcs = _run(sim, fn, src, hw, last)
        assert _golden_ok(r, out), (fn, name, hw, last, len(out), r[5])
        _check_crcs(src, hw, crcs)
    print("\n%s: %d runs, %d bytes, %.1f s" % (fn, len(sel), sum(len(cases[s[0]].data) for s in sel), time.time() - t))


@pytest.mark.parametrize("level", [2, 3])
def test_greedy_levels_on_traps(sim, traps, level):
    cases, _, runs = traps
    for name, hw, last, r in _select(runs, cases, level):
        src = cases[name].data
        out, crcs = _run(sim, "sim_deflate_level", src, hw, last, level)
        assert _golden_ok(r, out), (name, level, hw, last)
        _check_crcs(src, hw, crcs)


@pytest.mark.parametrize("level", [4, 5, 6, 7, 8, 9])
def test_lazy_levels_on_traps(sim, traps, level):
    """the lazy kernels (chains, per-position searches, serial parse) + K2.  The emulator is slow here: every run of
    up to 12 000 bytes, and at levels 6 and 9 every run of up to 40 000 (the chain budgets of 1024 / 4096 and the
    MAX_DIST cases live at 8 and 9; level 8's long runs are left to the GPU test)"""
    cases, _, runs = traps
    lim = 40000 if level in (6, 9) else 12000
    sel = _select(runs, cases, level, max_len=lim)
    if level == 8:
        sel += [s for s in _select(runs, cases, level) if s[0].startswith("f1_chain") and len(cases[s[0]].data) > lim]
    t = time.time()
    for name, hw, last, r in sel:
        src = cases[name].data
        out, crcs = _run(sim, "sim_deflate_lazy", src, hw, last, level)
        assert _golden_ok(r, out), (name, level, hw, last)
        _check_crcs(src, hw, crcs)
    print("\nlazy %d: %d runs, %d bytes, %.1f s" % (level, len(sel), sum(len(cases[s[0]].data) for s in sel), time.time() - t))


@pytest.mark.parametrize("level", [1, 3, 6])
def test_coalesced_launch_of_trap_requests(sim, traps, level):
    """trap inputs of up to 16 KiB as the requests of one coalesced launch (a request per slot of 16 KiB): each one's
    bytes are its own call's, i.e. the golden"""
    cases, _, runs = traps
    chunk = 16384
    reqs = [(name, r) for name, hw, last, r in _select(runs, cases, level, max_len=chunk) if last == 1 and hw >= chunk]
    slots, cdesc = [], []
    for name, _ in reqs:
        d = cases[name].data
        slots.append(d + bytes([0xEE]) * (chunk - len(d)))
        cdesc.append(len(d) | 0x80000000)
    buf = b"".join(slots); nch = len(cdesc)
    cd = np.array(cdesc, np.uint32); lens = np.zeros(nch, np.uint32); crcs = np.zeros(nch, np.uint32)
    out = C.create_string_buffer(len(buf) * 9 // 8 + 4096 * nch)
    total = sim.sim_deflate_ragged(buf, nch, chunk, cd.ctypes.data, level, out, lens.ctypes.data, crcs.ctypes.data)
    pos = 0
    for k, (name, r) in enumerate(reqs):
        ln = int(lens[k])
        assert _golden_ok(r, out.raw[pos:pos + ln]), (name, level)
        assert int(crcs[k]) == zlib.crc32(cases[name].data) & 0xffffffff, name
        pos += ln
    assert pos == total and len(reqs) > 50
