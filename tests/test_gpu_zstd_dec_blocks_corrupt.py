"""Corrupted many-block zstd frames on the GPU, all from committed fixtures: the sample of the emulator's sweep over the block
route (tests/golden/zstd_dec_blocks/corrupt_sample.json; tests/test_sim_zstdd_blocks_corrupt.py holds it against the sweep)
through qzd_zstd_decompress_frames_ex in calls of at most 512 segments, with a good frame - three of many blocks, one of one -
at the front, at the back and at every multiple of QZK_ZD_G: every line under route `blocks` with its count - the mutant's own
and, behind it, the base's stale one - and every mutant under route `frame`.  The device gives the {status, in_used, out_len}
the emulator pinned, every accepted output has its SHA, and the bytes between the segments are untouched.  No input reaches the
GPU whose answer was not first obtained on the CPU; each call runs once.  libzstd is not needed."""
import numpy as np
import pytest

import zstdd_blocks_mutate as X
import zstdd_blocks_sim as B
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


def device_call(ctx, call, counts, route):
    """[(frame, cap, tag)] -> ([(status, in_used, out_len)], [outputs], the bytes between the segments are still 0xEE)"""
    comp, segs, out_size = D.layout([c[0] for c in call], [c[1] for c in call], gap=GAP)
    d_in = ctx.alloc(len(comp) + 64); d_in.upload(comp)
    d_out = ctx.alloc(out_size + 64); d_out.upload(np.full(out_size + 64, 0xEE, np.uint8))
    res = ctx.zstd_decompress_frames(d_in, d_out, [tuple(int(x) for x in s) for s in segs], nblocks=counts, route=route)
    out = d_out.download(out_size + 64)
    d_in.free(); d_out.free()
    between = np.ones(out_size + 64, bool)
    for s in segs:
        between[int(s["out_off"]):int(s["out_off"]) + int(s["out_cap"])] = False
    outs = [out[int(s["out_off"]):int(s["out_off"]) + int(r["out_len"])].tobytes() for s, r in zip(segs, res)]
    return [(int(r["status"]), int(r["in_used"]), int(r["out_len"])) for r in res], outs, bool((out[between] == 0xEE).all())


def run(ctx, items, route):
    """items: (frame, cap, (what, pinned triple, sha or None, count)) -> how many were held against their pin"""
    good = X.neighbours()
    ncalls = held = 0
    for call in M.calls(items, good, M.GROUP):
        assert len(call) <= 512 and call[0][2] is None and call[-1][2] is None and all(c[2] is None for c in call[::M.GROUP])
        counts = [next(g[3] for g in good if g[0] is c[0]) if c[2] is None else c[2][3] for c in call]
        res, outs, clean = device_call(ctx, call, counts, route)
        assert clean, "bytes between the segments were written in call %d under route %s" % (ncalls, route)
        for (frame, cap, tag), r, o in zip(call, res, outs):
            if tag is None:
                g = next(g for g in good if g[0] is frame)
                assert r == (0, len(frame), g[1]) and M.sha(o) == g[2], ("a good neighbour", route, r)
                continue
            what, want, digest, count = tag
            assert r == want, (what, route, count, r, want)
            if r[0] == 0:
                assert M.sha(o) == digest, (what, route)
            held += 1
        ncalls += 1
    return held


def test_the_sample_under_both_counts_and_under_route_frame(ctx):
    assert M.GROUP == 4 and len(X.neighbours()) == 4
    rows = X.parse_sample(X.sample())
    by = X.base_by_name()
    assert sum(1 for r in rows if r[6]) >= 1000 and sum(1 for r in rows if not r[6] and r[4][0] == B.EHINT) >= 100
    assert len(set(r[0] for r in rows)) == len(by) == 38
    items = []
    for name, pos, value, count, want, digest, own in rows:
        assert (want[0] == 0) == (digest is not None)
        b = by[name]
        items.append((b.mutant(pos, value), b.cap, ("%s byte %d = %d" % (name, pos, value), want, digest, count)))
    assert run(ctx, items, "blocks") == len(rows)
    mine = [it for it, r in zip(items, rows) if r[6]]
    assert run(ctx, mine, "frame") == len(mine)
