"""The LZ4 level-1 compressors on trap inputs (tests/lz4_traps.py) without a GPU: every trap is live in liblz4 1.9.3's own
frame (tests/golden/lz4_traps/index.json holds its length and SHA-256), the oracle writes those bytes, and so do the kernel
bodies on the SIMT emulator (tests/sim/): qzk_lz4c_kernel, qzk_lz4c_pull_kernel with one and three waves (equal-size traps
as the frames of one call), the hardware-path header, the linked-block kernels, the pull kernel across the wrap of its
16-bit epoch and through a whole turn of it (child processes), and all three under AddressSanitizer in a stand-alone
program with every input in a heap buffer of exactly its size."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import lz4_traps as T
import oracle_lib as O
import refcalls as R

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)
INDEX = os.path.join(HERE, "golden", "lz4_traps", "index.json")


def sha(b):
    return hashlib.sha256(b).hexdigest()


def stride_of(fs):
    return (fs + 15 + 4 + 8 + 64 + 15) & ~15


@pytest.fixture(scope="module")
def traps():
    t = time.time()
    tr = T.all_traps()
    with open(INDEX) as f:
        idx = {e["name"]: e for e in json.load(f)["traps"]}
    print("\n%d traps, %d bytes, built in %.1f s" % (len(tr), sum(len(x.data) for x in tr), time.time() - t))
    return tr, idx


def pinned(idx, t, out):
    e = idx[t.name]
    return len(out) == e["frame_len"] and sha(out) == e["frame_sha256"]


def test_index_holds_every_trap_and_every_trap_is_live(traps):
    """inputs rebuild to the recorded SHA-256; with liblz4 1.9.3 at hand its frame is the recorded one and the check is
    evaluated again on it, otherwise the index carries the liveness recorded when it was written"""
    tr, idx = traps
    assert [t.name for t in tr] == list(idx) and len(tr) >= 150
    assert {t.family for t in tr} == set(T.FAMILIES)
    live = R.lz4_pinned()
    for t in tr:
        e = idx[t.name]
        assert (len(t.data), sha(t.data), t.family, t.mode) == (e["n"], e["input_sha256"], e["family"], e["mode"]), t.name
        assert e["live"] and e["decodes"] and e["model_agrees"], t.name
        if live:
            frame = R.lz4f_compress_frame(t.data, 1)
            assert pinned(idx, t, frame), t.name
            assert t.check(T.parse_frame(frame)[2]), (t.name, t.aim)
    for name, fired in T.G_FIRED.items():
        assert idx[name]["fired"] == fired, name


def test_model_reads_the_pinned_sequences(traps):
    """the serial restatement the traps are built with, against the sequence lists liblz4 wrote (whole where the index holds
    them whole)"""
    tr, idx = traps
    for t in tr:
        rec = idx[t.name]["seqs"]
        if isinstance(rec, dict):
            continue
        m = T.model(t.data)
        assert len(m) == len(rec), t.name
        for x, r in zip(m, rec):
            assert x[0] == bool(r[0]), t.name
            if not x[0]:
                assert [list(s) for s in x[1]] == r[3] and x[2] == r[2], t.name


def test_oracle_on_every_trap(traps):
    """oracle/qzo_lz4.c, the restatement most tests compare with, meets liblz4 off the corpora"""
    tr, idx = traps
    for t in tr:
        n = len(t.data)
        rc, _, out, _ = O.sw_compress("LZ4", t.data, 65536, 1, cap=n + n // 255 + 4096)
        assert rc == 0 and pinned(idx, t, out), (t.name, t.aim)


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
    return load_sim(so)


def load_sim(so):
    S = C.CDLL(so)
    S.sim_lz4c.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    S.sim_lz4c_hw.argtypes = S.sim_lz4c.argtypes
    S.sim_lz4c_pull.argtypes = S.sim_lz4c.argtypes + [C.c_uint32]
    S.sim_lz4c_linked.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    S.sim_lz4c_linked_many.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    return S


def run_group(S, fn, group, fs, waves=None):
    """equal-size traps as the frames of one call -> the frames"""
    src = b"".join(t.data for t in group)
    nfr = max(1, len(group)) if fs else 1
    fs = fs or 65536                                      # the empty input: one call, one (empty) frame
    stride = stride_of(fs)
    slots = np.zeros(nfr * stride + 64, np.uint8); lens = np.zeros(nfr, np.uint32)
    args = [src, len(src), fs, slots.ctypes.data, stride, lens.ctypes.data]
    getattr(S, fn)(*(args + ([waves] if waves else [])))
    return [bytes(slots[i * stride:i * stride + int(lens[i])]) for i in range(nfr)]


def check_groups(S, fn, traps, waves=None):
    tr, idx = traps
    t0 = time.time(); nb = 0
    for fs, group in T.by_size(tr).items():
        outs = run_group(S, fn, group, fs, waves)
        for t, out in zip(group, outs):
            assert pinned(idx, t, out), (fn, waves, t.name, t.aim, len(out), idx[t.name]["frame_len"])
        nb += fs * len(group)
    print("\n%s%s: %d bytes in %.1f s" % (fn, " (%d waves)" % waves if waves else "", nb, time.time() - t0))


def test_lds_table_kernel_on_block_traps(sim, traps):
    check_groups(sim, "sim_lz4c", traps)


@pytest.mark.parametrize("waves", [1, 3])
def test_pull_kernel_on_block_traps(sim, traps, waves):
    check_groups(sim, "sim_lz4c_pull", traps, waves)


def test_hardware_path_header_on_a_subset(sim, traps):
    """two traps per family behind qzLZ4HeaderGen's header: only the header differs (test_lz4_hardware_path_header)"""
    tr, idx = traps
    seen = {}
    for t in tr:
        if t.mode == "block" and len(t.data) <= 16384 and len(t.data) > 0 and len(seen.setdefault(t.family, [])) < 2:
            seen[t.family].append(t)
    for fam, ts in seen.items():
        for t in ts:
            out = run_group(sim, "sim_lz4c_hw", [t], len(t.data))[0]
            desc = bytes([0x4C, 0x40]) + len(t.data).to_bytes(8, "little")
            hdr = bytes([0x04, 0x22, 0x4D, 0x18]) + desc + bytes([(O.lib().qzo_xxh32(desc, len(desc), 0) >> 8) & 0xff])
            assert out[:15] == hdr, t.name
            e = idx[t.name]
            sw = O.sw_compress("LZ4", t.data, 65536, 1, cap=len(t.data) + 4096)[2]
            assert pinned(idx, t, sw) and out[15:] == sw[15:] and len(out) == e["frame_len"], t.name


def test_linked_kernels_on_linked_traps(sim, traps):
    tr, idx = traps
    linked = [t for t in tr if t.mode == "linked"]
    assert len(linked) >= 8
    for t in linked:
        n = len(t.data)
        out = C.create_string_buffer(n + n // 255 + 4096); ol = C.c_uint32(0)
        sim.sim_lz4c_linked(t.data, n, out, C.byref(ol))
        assert pinned(idx, t, out.raw[:ol.value]), (t.name, t.aim)
    # two of them as the chunks of one launch of the many-frames kernel
    two = [t for t in linked if len(t.data) == 65536 + 8192][:2]
    chunk = 65536 + 8192
    stride = (chunk + 15 + 4 * 2 + 8 + 64 + 15) & ~15
    slots = C.create_string_buffer(2 * stride); lens = (C.c_uint32 * 2)()
    sim.sim_lz4c_linked_many(b"".join(t.data for t in two), 2 * chunk, chunk, 2, slots, stride, lens)
    for k, t in enumerate(two):
        assert pinned(idx, t, slots.raw[k * stride:k * stride + lens[k]]), t.name


CHILD = r"""
import sys
sys.path.insert(0, %r)
import test_sim_lz4_traps as M, lz4_traps as T, json
S = M.load_sim(%r)
tr = T.all_traps()
idx = {e["name"]: e for e in json.load(open(M.INDEX))["traps"]}
bad = []
for fs, group in T.by_size(tr).items():
    if fs > 16384:
        continue
    for t, out in zip(group, M.run_group(S, "sim_lz4c_pull", group, fs, 1)):
        if not M.pinned(idx, t, out):
            bad.append(t.name)
print("frames", sum(len(g) for fs, g in T.by_size(tr).items() if fs <= 16384), "bad", bad)
sys.exit(1 if bad else 0)
"""


def test_pull_kernel_across_the_epoch_wrap(sim, traps):
    """one wave, its epoch started 60 frames short of 65535 (the driver reads QZSIM_LZ4_EPOCH0 once per process, hence the
    child): the table is cleared again in the middle of the trap list and every frame stays the pinned one"""
    env = dict(os.environ, QZSIM_LZ4_EPOCH0=str(65535 - 60))
    r = subprocess.run([sys.executable, "-c", CHILD % (HERE, os.path.join(SIMDIR, "libqzsim.so"))], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "bad []" in r.stdout, r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 100


TURN_CHILD = r"""
import sys
sys.path.insert(0, %r)
import test_sim_lz4_traps as M, lz4_traps as T, json
S = M.load_sim(%r)
tr = {t.name: t for t in T.all_traps()}
idx = {e["name"]: e for e in json.load(open(M.INDEX))["traps"]}
plant, probes = tr["e_epoch_plant"], [tr["e_epoch_probe%%d" %% k] for k in (1, 2, 3)]
tiny = T.rnd(16, 77)                    # probes 1..4 are live: every tiny frame plants its words, always in the same slots
hw = {T.hash4(T.u32(w, 0)) for w in T.EPOCH_WORDS}
assert len(hw) == 3 and all(T.hash4(T.u32(tiny, f)) not in hw for f in range(1, 5))
bad = []
if not M.pinned(idx, plant, M.run_group(S, "sim_lz4c_pull", [plant], 4096, 1)[0]):      # the wave's epoch 1
    bad.append("plant")
N = 65532                               # epochs 2 .. 65533
class Tiny: data = tiny
outs = M.run_group(S, "sim_lz4c_pull", [Tiny] * N, 16, 1)
if len(set(outs)) != 1:
    bad.append("tiny")
# epochs 65534, 65535 and the one behind the wrap - or, if the epoch turned early, the plant frame's own epoch again
for t, out in zip(probes, M.run_group(S, "sim_lz4c_pull", probes, 4096, 1)):
    if not M.pinned(idx, t, out):
        bad.append(t.name)
print("frames", N + 4, "bad", bad)
sys.exit(1 if bad else 0)
"""


def test_pull_kernel_through_a_whole_turn_of_the_epoch(sim, traps):
    """one wave in a fresh child: e_epoch_plant (epoch 1), 65532 tiny frames of 16 bytes, then e_epoch_probe1..3 - at the
    last two epochs before the wrap and the first behind it, each with a word of its own.  A table that is not cleared when the epoch starts again
    still holds the plant frame's entries under a live epoch; a probe frame then matches a word it does not have at 30..38.
    Every frame must be liblz4's."""
    r = subprocess.run([sys.executable, "-c", TURN_CHILD % (HERE, os.path.join(SIMDIR, "libqzsim.so"))],
                       env={k: v for k, v in os.environ.items() if k != "QZSIM_LZ4_EPOCH0"}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bad []" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_no_overreads_under_sanitizers(tmp_path, traps):
    """tests/sim/sim_lz4traps.cpp, a program of its own: every trap input in a heap buffer of exactly n bytes, the three
    compressors on it, built with -fsanitize=address,undefined - a probe, a window load or a count that reads past a
    block's end ends the program.  Nothing sanitized is loaded into python."""
    tr, idx = traps
    blob = tmp_path / "traps.bin"
    with open(blob, "wb") as f:
        for t in tr:
            f.write(len(t.data).to_bytes(4, "little") + t.data)
    exe = str(tmp_path / "sim_lz4traps_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", SIMDIR, "-Wno-unused-function", "-o", exe, os.path.join(SIMDIR, "sim_lz4traps.cpp")])
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and ("%d inputs, 0 failures" % len(tr)) in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
