"""Corrupted and hand-built zstd frames on the GPU, all from committed fixtures (tests/golden/zstd_dec_corrupt/, made by
tests/golden/gen_zstd_dec_corrupt.py): every hand-built frame and the committed sample of the emulator's corruption sweep
(tests/test_sim_zstdd_corrupt.py holds the sample against the sweep) through qzd_zstd_decompress_frames in calls of at most
512 segments, with a good frame at the front, at the back and at every multiple of QZK_ZD_G.  The device gives the
{status, in_used, out_len} the emulator pinned, every accepted output has its SHA, and the bytes between the segments are
untouched.  No input reaches the GPU whose answer was not first obtained on the CPU.  libzstd is not needed."""
import numpy as np
import pytest

import zstdd_mutate as M
import zstdd_sim as D
import qatzip_amd

pytestmark = pytest.mark.gpu

GAP = 48                            # between two segments' outputs, and in front of the first: no multiple of 16 either side


@pytest.fixture(scope="module")
def ctx():
    c = qatzip_amd.Context(0)
    yield c
    c.close()


def device_call(ctx, call):
    """[(frame, cap, tag)] -> ([(status, in_used, out_len)], [outputs], the bytes between the segments are still 0xEE)"""
    comp, segs, out_size = D.layout([c[0] for c in call], [c[1] for c in call], gap=GAP)
    d_in = ctx.alloc(len(comp) + 64); d_in.upload(comp)
    d_out = ctx.alloc(out_size + 64); d_out.upload(np.full(out_size + 64, 0xEE, np.uint8))
    res = ctx.zstd_decompress_frames(d_in, d_out, [tuple(int(x) for x in s) for s in segs])
    out = d_out.download(out_size + 64)
    d_in.free(); d_out.free()
    between = np.ones(out_size + 64, bool)
    for s in segs:
        between[int(s["out_off"]):int(s["out_off"]) + int(s["out_cap"])] = False
    outs = [out[int(s["out_off"]):int(s["out_off"]) + int(r["out_len"])].tobytes() for s, r in zip(segs, res)]
    return [(int(r["status"]), int(r["in_used"]), int(r["out_len"])) for r in res], outs, bool((out[between] == 0xEE).all())


def test_hand_built_frames_and_the_sample_between_good_frames(ctx):
    hand = M.hand_index()
    sample = M.parse_sample(hand["sample"])
    assert len(hand["frames"]) >= 38 and len(sample) >= 100
    by = M.base_by_name()
    items = []
    for e in hand["frames"]:
        items.append((M.hand_bytes(e), e["content"] + 64, ("hand:" + e["name"], tuple(e["sim"]), e.get("sha256"))))
    for name, pos, value, r, digest in sample:
        b = by[name]
        assert (r[0] == 0) == (digest is not None)          # an accepted mutant is in the sample for its other bytes
        items.append((b.mutant(pos, value), b.cap, ("%s byte %d = %d" % (name, pos, value), r, digest)))
    good = M.neighbours()
    big = next(e for e in D.index()["frames"] if e["name"] == "a_text_300000_L19_cs")
    front = (D.frame_bytes(big), big["content"], big["sha256"])
    shas = {id(g[0]): g for g in good + [front]}
    ncalls = nmut = 0
    for call in M.calls(items, good, M.GROUP, extra_front=front):
        assert len(call) <= 512 and call[0][2] is None and call[-1][2] is None and all(c[2] is None for c in call[::M.GROUP])
        res, outs, clean = device_call(ctx, call)
        assert clean, "bytes between the segments were written in call %d" % ncalls
        for (frame, cap, tag), r, o in zip(call, res, outs):
            if tag is None:
                g = shas[id(frame)]
                assert r == (0, len(frame), g[1]) and M.sha(o) == g[2], ("a good neighbour", r)
                continue
            what, want, digest = tag
            assert r == want, (what, r, want)
            if r[0] == 0:
                assert M.sha(o) == digest, what
            nmut += 1
        ncalls += 1
    assert nmut == len(items)
