"""GPU: the LZ4 frame decoders (qzk_lz4.h) and the copy engine (qzk_lz_batch.h) sequence by sequence - the matrix of
tests/lz4_blocks_cases.py on the one-wave route and a wave per block, against the builder's byte-by-byte model and what
liblz4 1.9.3 answered (tests/golden/lz4_sequences/index.json; liblz4 itself is not needed here).  What the CPU twin
(tests/test_sim_lz4_sequences.py) cannot see is met here: the order of LDS accesses between lanes, matches read from
memory the wave has only just stored, the direct paths reading what other lanes wrote."""
import hashlib
import json
import os

import numpy as np
import pytest

import lz4_blocks_cases as K
from qatzip_amd import api as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "lz4_sequences", "index.json")) as f:
    INDEX = {c["name"]: c for c in json.load(f)["cases"]}
CASES = K.cases()
GUARD = 67
# (wrapping, route): every frame on the kernels it is built for, and the blocks-route frames on the one-wave kernel as well
RUNS = (("wave", "wave"), ("blocks", "blocks"), ("blocks", "wave"))


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
def frames():
    """{(case name, wrapping): frame}, built once and held against the index"""
    out = {}
    assert [c.name for c in CASES] == list(INDEX)
    for c in CASES:
        assert INDEX[c.name]["class"] == c.cls
        for w in c.wrappings():
            fr, r = c.frame(w), INDEX[c.name][w]
            assert len(fr) == r["len"] and _sha(fr) == r["sha"] and c.cap(w) == r["cap"], (c.name, w)
            out[c.name, w] = fr
    return out


def decode(ctx, frames, caps, route, phase=K.PHASE, per_block=False):
    """the frames as the segments of ONE call; every output `phase` bytes off a 16-byte boundary, at least GUARD bytes of 0xA5
    behind every out_cap -> [(status, in_used, out_len, output bytes or None)]; the guards are checked here.  per_block:
    every frame goes a wave per block, where a frame that does not fit is refused before a byte of it is written"""
    comp = b"".join(frames)
    segs, io, oo = [], 0, phase
    for fr, cap in zip(frames, caps):
        segs.append((io, oo, len(fr), cap))
        io += len(fr); oo += (cap + GUARD + 15) & ~15
    d_c = ctx.alloc(len(comp)); d_c.upload(comp)
    d_o = ctx.alloc(oo + 16); d_o.upload(np.full(oo + 16, 0xA5, np.uint8))
    try:
        res = ctx.lz4_decompress_frames(d_c, d_o, segs, route=route)
        out = d_o.download(oo + 16)
    finally:
        d_c.free(); d_o.free()
    assert (out[:phase] == 0xA5).all()
    got = []
    for i, (_, o, _, cap) in enumerate(segs):
        end = segs[i + 1][1] if i + 1 < len(segs) else out.size
        assert (out[o + cap:end] == 0xA5).all(), ("a store beyond out_cap", i, route)
        st = int(res[i]["status"])
        if st == -2 and per_block:
            assert (out[o:o + cap] == 0xA5).all(), ("output of a frame that does not fit", i)
        got.append((st, int(res[i]["in_used"]), int(res[i]["out_len"]), out[o:o + int(res[i]["out_len"])].tobytes() if st == 0 else None))
    return got


@pytest.fixture(scope="module")
def decoded(ctx, frames):
    """every run of RUNS, one call each: {(wrapping, route): {case name: result}}"""
    out = {}
    for w, route in RUNS:
        cs = [c for c in CASES if w in c.wrappings()]
        got = decode(ctx, [frames[c.name, w] for c in cs], [c.cap(w) for c in cs], route, per_block=w == "blocks" and route != "wave")
        out[w, route] = {c.name: g for c, g in zip(cs, got)}
    return out


def test_the_matrix_on_both_routes(decoded, frames):
    """every case of the matrix; all failures are named, not the first only"""
    failed = []
    for c in CASES:
        verdicts = set()
        for w, route in RUNS:
            if w not in c.wrappings():
                continue
            st, used, olen, out = decoded[w, route][c.name]
            try:
                K.check(c, w, INDEX[c.name][w], frames[c.name, w], st, used, olen, out, (w, route))
            except AssertionError as e:
                failed.append(e.args[0] if e.args else (c.name, w, route))
            verdicts.add(st)
        if len(verdicts) != 1:                                      # the verdict does not depend on the route
            failed.append((c.name, "verdicts", sorted(verdicts)))
    assert not failed, failed


@pytest.mark.parametrize("cls", K.CLASSES)
def test_every_class_is_decided_as_the_index_says(decoded, cls):
    """the classes one by one, so that a failure says which decision it is about: strict cases follow liblz4, the two exempt
    classes are this decoder's own decisions"""
    cs = [c for c in CASES if c.cls == cls]
    assert cs
    for c in cs:
        for w, route in RUNS:
            if w not in c.wrappings():
                continue
            st = decoded[w, route][c.name][0]
            if cls == K.OFFSET0:
                assert st != 0, (c.name, w, route)
            elif cls == K.LENIENT:
                assert st == 0, (c.name, w, route)
            elif c.cap_delta >= 0:
                assert (st == 0) == (INDEX[c.name][w]["liblz4"] == "OK"), (c.name, w, route, st)
            else:
                assert st == -2, (c.name, w, route, st)


@pytest.mark.parametrize("phase", range(16))
def test_every_output_phase(ctx, frames, phase):
    """one case per path with its output at every phase of a 16-byte row: the first row, `hd`, the masked flush"""
    reps = K.representatives()
    assert len(reps) == 4
    for w, route in RUNS:
        got = decode(ctx, [frames[c.name, w] for c in reps], [c.cap(w) for c in reps], route, phase=phase,
                     per_block=w == "blocks" and route != "wave")
        for c, (st, used, olen, out) in zip(reps, got):
            K.check(c, w, INDEX[c.name][w], frames[c.name, w], st, used, olen, out, (w, route, phase))


def test_capacities_at_every_phase(ctx, frames):
    """the capacity cases (exact, one more, one less, 17 less) of every path once more at the phases 0 and 15"""
    cs = [c for c in CASES if c.name.startswith("cap_")]
    assert len(cs) == 16
    for phase in (0, 15):
        for w, route in RUNS:
            got = decode(ctx, [frames[c.name, w] for c in cs], [c.cap(w) for c in cs], route, phase=phase,
                         per_block=w == "blocks" and route != "wave")
            for c, (st, used, olen, out) in zip(cs, got):
                K.check(c, w, INDEX[c.name][w], frames[c.name, w], st, used, olen, out, (w, route, phase))


def test_a_subset_through_qzdecompress(frames):
    """one case per path and per class through the session API: QZ_OK with the bytes, or QZ_FAIL with nothing"""
    names = [c.name for c in K.representatives()]
    names += ["cap_batch_minus1", "cap_direct_match_minus17", "mem_25_then_window", "win_dist3_len_4_7_8_9_31_32_33_300",
              "chain_depth63", "bad_offset_above_produced_by_1", "bad_cut_in_ml_ext", "end_closing_literals_0",
              "end_ml_ext_in_last_5", "offset0", "direct_match_offset0", "hist_linked_reach_65535", "hist_independent_reach_33"]
    by = {c.name: c for c in CASES}
    assert {by[n].cls for n in names} == set(K.CLASSES)
    s = A.Session(lz4=True)
    assert s.rc_setup == A.QZ_OK
    try:
        for n in names:
            c = by[n]
            for w in c.wrappings():
                fr = frames[n, w]
                want = K.expect(c, w, INDEX[n][w])
                rc, used, back = s.decompress(fr, c.cap(w))
                if want[0] == "ok":
                    assert rc == A.QZ_OK and used == len(fr) and bytes(back) == want[1], (n, w, rc)
                else:
                    assert rc == A.QZ_FAIL and used == 0 and len(back) == 0, (n, w, rc)
    finally:
        s.close()
