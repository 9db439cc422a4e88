"""The LZ4-HC kernels (qatzip_amd/csrc/qzk_lz4hc.h) on the trap inputs of tests/lz4hc_traps.py without a GPU: every trap is
live in liblz4 1.9.3's own frame at every level of its `levels` (tests/golden/lz4hc_traps/index.json holds length, SHA-256,
liveness and the decision labels of the serial model's trace), and the kernel bodies write those bytes on the SIMT emulator
(tests/sim/sim_lz4hc.cpp) - equal-size traps as the frames of one call, linked traps in rounds of all, one and two blocks,
a block of a linked frame alone, the hardware-path header - and run under AddressSanitizer in a stand-alone program with
every input in a heap buffer of exactly its size.  The -m gpu twin is tests/test_gpu_lz4hc_traps.py."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess

import pytest

import lz4_traps as L1
import lz4hc_traps as T
import refcalls as R
from test_sim_lz4hc import SIMDIR, _load, _pool, sim_frames, simso  # noqa: F401  (simso: the fixture that builds the emulator)

HERE = os.path.dirname(os.path.abspath(__file__))
INDEX = os.path.join(HERE, "golden", "lz4hc_traps", "index.json")
HW_HEAD = bytes([0x04, 0x22, 0x4D, 0x18, 0x4C, 0x40])
SEARCH_SEEDS = range(100000, 100150)        # the short run of the state-machine search against the library


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def traps():
    tr = T.all_traps()
    with open(INDEX) as f:
        doc = json.load(f)
    return tr, {e["name"]: e for e in doc["traps"]}, doc


def pinned(idx, t, lvl, out):
    e = idx[t.name]["levels"][str(lvl)]
    return len(out) == e["frame_len"] and sha(out) == e["frame_sha256"]


def split_frames(blob, n):
    """the n frames of one call's output (each ends in an end mark and a content checksum)"""
    out, pos = [], 0
    for _ in range(n):
        p = pos + (15 if blob[pos + 4] & 8 else 7)
        while True:
            w = struct.unpack_from("<I", blob, p)[0]; p += 4
            if w == 0:
                break
            p += w & 0x7fffffff
        out.append(blob[pos:p + 4]); pos = p + 4
    assert pos == len(blob)
    return out


def test_index_holds_every_trap_and_every_trap_is_live(traps):
    """inputs rebuild to the recorded SHA-256 and every trap is live at every level; with liblz4 1.9.3 at hand the block traps'
    frames are made again, the model writes the same bytes and the check is evaluated again on them (the linked traps:
    test_model_and_library_on_linked_traps)"""
    tr, idx, doc = traps
    assert [t.name for t in tr] == list(idx) and len(tr) >= 90
    assert {t.family for t in tr} == set(T.FAMILIES) and doc["labels"] == list(T.LABELS)
    assert 8 <= sum(1 for t in tr if T.is_linked(t)) <= 14
    assert all(len(t.data) <= 4096 for t in tr if not T.is_linked(t)) and len(T.by_size(tr)) <= 24
    for t in tr:
        e = idx[t.name]
        assert (len(t.data), sha(t.data), t.family) == (e["n"], e["input_sha256"], e["family"]), t.name
        assert list(e["levels"]) == [str(x) for x in t.levels] and {3, 8} <= set(t.levels), t.name
        assert t.family != "B" or t.levels == T.LEVELS, t.name
        for lvl in t.levels:
            assert e["levels"][str(lvl)]["live"], (t.name, lvl)
            if R.lz4_pinned() and not T.is_linked(t):
                frame = R.lz4f_compress_frame(t.data, lvl)
                assert pinned(idx, t, lvl, frame), (t.name, lvl)
                mframe, trace = T.model(t.data, lvl)
                assert mframe == frame, (t.name, lvl, "the model differs from liblz4")
                assert sorted(doc["labels"][i] for i in e["levels"][str(lvl)]["labels"]) == trace.labels(), (t.name, lvl)
                assert t.check(L1.parse_frame(frame)[2], trace, lvl), (t.name, lvl, t.aim)


def test_every_label_is_fired_by_a_live_trap(traps):
    """the census, counted again from the index: every decision label of the model is in the trace of a live trap, but those
    lz4hc_traps.UNREACHABLE argues away - at most three"""
    tr, idx, doc = traps
    census = {lab: 0 for lab in T.LABELS}
    for e in idx.values():
        seen = set()
        for rec in e["levels"].values():
            if rec["live"]:
                seen |= {doc["labels"][i] for i in rec["labels"]}
        for lab in seen:
            census[lab] += 1
    assert census == doc["census"]
    silent = sorted(lab for lab, c in census.items() if c == 0)
    assert silent == sorted(T.UNREACHABLE) and len(silent) <= 3, silent
    assert T.__doc__ and all(lab in T.LABELS for lab in T.UNREACHABLE)


def test_block_traps_one_call_per_size_and_level(simso, traps):
    """per size class and level one sim_lz4hc call whose frames are that class's traps (frame_sz is the size class)"""
    tr, idx, _ = traps
    for fs, group in T.by_size(tr).items():
        for lvl in T.LEVELS:
            todo = [t for t in group if lvl in t.levels]
            outs = split_frames(sim_frames(simso, b"".join(t.data for t in todo), lvl, frame_sz=fs or None), len(todo))
            for t, out in zip(todo, outs):
                assert pinned(idx, t, lvl, out), (t.name, lvl, t.aim, len(out), idx[t.name]["levels"][str(lvl)]["frame_len"])


def test_block_traps_behind_the_hardware_path_header(simso, traps):
    """the same calls with qzLZ4HeaderGen's header (FLG 0x4C whatever the size), levels 3 and 8: behind the 15 header bytes
    every frame is the pinned one"""
    tr, idx, _ = traps
    for fs, group in T.by_size(tr).items():
        if fs == 0:
            continue
        for lvl in (3, 8):
            blob = sim_frames(simso, b"".join(t.data for t in group), lvl, frame_sz=fs, hw=1)
            pos = 0
            for t in group:
                e = idx[t.name]["levels"][str(lvl)]
                assert blob[pos:pos + 6] == HW_HEAD and blob[pos + 6:pos + 14] == fs.to_bytes(8, "little"), t.name
                body = blob[pos + 15:pos + e["frame_len"]]
                assert len(body) == e["frame_len"] - 15, t.name
                # the pinned frame's own header: FLG with the size bit, the block-independence bit at or below 64 KB
                desc = bytes([0x6C, 0x40]) + fs.to_bytes(8, "little")
                head = b"\x04\x22\x4d\x18" + desc + bytes([(T.xxh32(desc) >> 8) & 0xff])
                assert sha(head + body) == e["frame_sha256"], (t.name, lvl)
                pos += e["frame_len"]
            assert pos == len(blob)


def _linked_job(arg):
    """one linked trap at one level in a worker: None, or what went wrong"""
    so, name, lvl, what = arg
    t = next(x for x in T.all_traps() if x.name == name)
    with open(INDEX) as f:
        idx = {e["name"]: e for e in json.load(f)["traps"]}
    e = idx[name]["levels"][str(lvl)]
    if what == "hw":
        blob = sim_frames(so, t.data, lvl, frame_sz=65536, hw=1)
        pos = 0
        for i, ch in enumerate(e["hw65536"]):
            piece = t.data[i * 65536:(i + 1) * 65536]
            body = blob[pos + 15:pos + 15 + ch["len"]]
            if blob[pos:pos + 14] != HW_HEAD + len(piece).to_bytes(8, "little") or len(body) != ch["len"] or sha(body) != ch["sha"]:
                return (name, lvl, "hw_buff_sz 65536, chunk %d" % i)
            pos += 15 + ch["len"]
        if pos != len(blob):
            return (name, lvl, "hw_buff_sz 65536, length")
        # above 64 KB liblz4's own FLG is 0x4C too: at hw_buff_sz 262144 the trap is one chunk and its frame the pinned one
        return None if pinned(idx, t, lvl, sim_frames(so, t.data, lvl, frame_sz=262144, hw=1)) else (name, lvl, "hw_buff_sz 262144")
    frame = sim_frames(so, t.data, lvl, batch=what)
    if not pinned(idx, t, lvl, frame):
        return (name, lvl, "rounds of %d" % what, t.aim)
    if what == 0 and t.family == "A":
        S = _load(so)
        pos, nb = 15, (len(t.data) + 65535) // 65536
        for k in range(nb):
            w = struct.unpack_from("<I", frame, pos)[0]
            blk = frame[pos:pos + 4 + (w & 0x7fffffff)]
            pos += len(blk)
            if k == 0:
                continue
            slot = C.create_string_buffer(S.sim_lz4hc_stride())
            ln = S.sim_lz4hc_block(t.data, len(t.data), len(t.data), lvl, k, slot)
            if slot.raw[:ln - (8 if k == nb - 1 else 0)] != blk:
                return (name, lvl, "block %d alone" % k)
    return None


def test_linked_traps_rounds_blocks_alone_and_hardware_header(simso, traps):
    """Every linked trap at levels 3 and 8 in one round; level 3 again in rounds of one block and level 8 in rounds of two.
    Family A's traps also through sim_lz4hc_block: block k >= 1, its chains and its parse made by a launch that sees nothing
    of the other blocks' work, is the block at that place of the pinned frame.  Every third trap behind the hardware path's
    header: at hw_buff_sz 65536 a frame per 64 KB chunk against the per-chunk records, at 262144 one chunk.  (Spread over
    worker processes as in test_sim_lz4hc.py: the emulator runs one launch at a time per process.)"""
    tr, idx, _ = traps
    linked = [t for t in tr if T.is_linked(t)]
    assert sum(1 for t in linked if t.family == "A") >= 9
    work = []
    for t in linked:
        assert t.levels == T.LINKED_LEVELS
        work += [(simso, t.name, 3, 0), (simso, t.name, 8, 0), (simso, t.name, 3, 1), (simso, t.name, 8, 2)]
    work += [(simso, t.name, lvl, "hw") for t in linked[::3] for lvl in (3, 8)]
    with _pool() as p:
        bad = [r for r in p.imap_unordered(_linked_job, work, chunksize=1) if r]
    assert not bad, bad


@pytest.mark.skipif(not R.lz4_pinned(), reason="liblz4 1.9.3 is not installed here")
def test_model_and_library_on_linked_traps(traps):
    """levels 3 and 8: the model writes liblz4's bytes, the trace holds the recorded labels and the check holds on liblz4's
    own frame"""
    tr, idx, doc = traps
    for t in tr:
        if not T.is_linked(t):
            continue
        for lvl in (3, 8):
            frame = R.lz4f_compress_frame(t.data, lvl)
            assert pinned(idx, t, lvl, frame), (t.name, lvl)
            mframe, trace = T.model(t.data, lvl)
            assert mframe == frame, (t.name, lvl, "the model differs from liblz4")
            assert sorted(doc["labels"][i] for i in idx[t.name]["levels"][str(lvl)]["labels"]) == trace.labels(), (t.name, lvl)
            assert t.check(L1.parse_frame(frame)[2], trace, lvl), (t.name, lvl, t.aim)


@pytest.mark.skipif(not R.lz4_pinned(), reason="liblz4 1.9.3 is not installed here")
def test_a_short_run_of_the_search_against_the_library(simso):
    """fresh seeds of the state-machine search: model, library and emulator agree on every input visited, and the run sees
    most of the state machine's labels again"""
    seen = set()
    for seed in SEARCH_SEEDS:
        n = T.SM_SIZES[seed & 1]
        src = T.sm_input(seed, n)
        lvl = 3 + seed % 6
        frame = R.lz4f_compress_frame(src, lvl)
        mframe, trace = T.model(src, lvl)
        assert mframe == frame, (seed, n, lvl)
        assert sim_frames(simso, src, lvl) == frame, (seed, n, lvl)
        seen |= set(trace.labels())
    assert "asc.opt" not in seen and len(seen) >= 30, sorted(seen)


def test_no_overreads_under_sanitizers(tmp_path, traps):
    """tests/sim/sim_lz4hc.cpp as a program of its own (SIM_LZ4HC_MAIN): every trap input in a heap buffer of exactly n bytes,
    level 3 in rounds of one block and level 8 in one round, built with -fsanitize=address,undefined - a search that reads a word
    at ilow + longest - 1 or at s - 65535 outside the input, a count or a chain trip that runs past its end, ends the
    program.  Nothing sanitized is loaded into python."""
    tr, idx, _ = traps
    shards = [[t for t in tr if not T.is_linked(t)]] + [[t] for t in tr if T.is_linked(t)]
    exe = str(tmp_path / "sim_lz4hc_san")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSIM_LZ4HC_MAIN",
                           "-I", SIMDIR, "-Wno-unused-function", "-o", exe, os.path.join(SIMDIR, "sim_lz4hc.cpp")])
    for i, shard in enumerate(shards):
        with open(tmp_path / ("traps%d.bin" % i), "wb") as f:
            for t in shard:
                f.write(len(t.data).to_bytes(4, "little") + t.data)
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    todo, running, ran = list(enumerate(shards)), [], 0
    while todo or running:                                  # the shards as processes of their own, a few at a time
        while todo and len(running) < max(1, min(8, cpus)):
            i, shard = todo.pop()
            running.append((shard, subprocess.Popen([exe, str(tmp_path / ("traps%d.bin" % i))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
        shard, proc = running.pop(0)
        out, err = proc.communicate(timeout=900)
        assert proc.returncode == 0 and ("%d inputs, 0 failures" % len(shard)) in out, ([t.name for t in shard][:3], out[-2000:], err[-4000:])
        ran += len(shard)
    assert ran == len(tr)
