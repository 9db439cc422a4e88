"""The block route of the zstd decoder on the GPU (qzd_zstd_decompress_frames_ex, include/qzamd_zstd_blocks.h): the committed
multi-block frames of tests/golden/zstd_dec_blocks/ give the {status, in_used, out_len} and the bytes the CPU emulator pinned
for the same kernels, routed and unrouted frames share a call, a zstd decode session reads a 40-block frame from the host,
the device's block count is the host's, and one 16 MiB frame of 128 blocks decodes alike under both routes."""
import hashlib
import os
import sys

import pytest

import datagen
import zstd_ref
import zstd_sim as S
import zstdd_blocks_sim as B
import zstdd_sim as D
import qatzip_amd
from qatzip_amd import api as A
from qatzip_amd._lib import zstd_bound

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_zstd_dec_blocks as G  # noqa: E402

pytestmark = pytest.mark.gpu


def _sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def ctx():
    c = qatzip_amd.Context(0)
    yield c
    c.zstd_decode_route("auto")
    c.close()


@pytest.fixture(scope="module")
def idx():
    return B.index()


def device_decode(ctx, frames, caps, nblocks, route):
    """the frames back to back, their outputs back to back -> ([(status, in_used, out_len)], [outputs])"""
    comp, segs, out_size = D.layout(frames, caps)
    d_in = ctx.alloc(len(comp) + 64); d_in.upload(comp)
    d_out = ctx.alloc(out_size + 64)
    res = ctx.zstd_decompress_frames(d_in, d_out, [tuple(int(x) for x in s) for s in segs], nblocks=nblocks, route=route)
    out = d_out.download(out_size).tobytes()
    d_in.free(); d_out.free()
    outs = [out[int(s["out_off"]):int(s["out_off"]) + int(r["out_len"])] for s, r in zip(segs, res)]
    return [(int(r["status"]), int(r["in_used"]), int(r["out_len"])) for r in res], outs


def test_every_committed_case_in_one_call(ctx, idx):
    cases = idx["cases"]
    assert len(cases) >= 35
    res, outs = device_decode(ctx, [B.frame_bytes(e) for e in cases], [e["cap"] for e in cases], [e["nblocks"] for e in cases], "blocks")
    for e, r, o in zip(cases, res, outs):
        assert list(r) == e["sim"], (e["name"], r)
        if r[0] == 0:
            assert _sha(o) == e["sha256"], e["name"]
    # route `frame` does not look at the counts: the same answers, but for the wrong counts
    res1, outs1 = device_decode(ctx, [B.frame_bytes(e) for e in cases], [e["cap"] for e in cases], [e["nblocks"] for e in cases], "frame")
    for e, r, r1, o, o1 in zip(cases, res, res1, outs, outs1):
        if r[0] == B.EHINT:
            assert r1 == (0, e["size"], e["cap"]), e["name"]
        else:
            assert (r1, o1) == (r, o), e["name"]


def test_the_frames_of_zstd_dec_through_route_blocks(ctx):
    entries = [e for e in D.index()["frames"] if B.walk_count(D.frame_bytes(e))]
    frames = [D.frame_bytes(e) for e in entries]
    res, outs = device_decode(ctx, frames, [e["content"] for e in entries], [B.walk_count(f) for f in frames], "blocks")
    for e, r, o in zip(entries, res, outs):
        assert list(r) == e["sim"], (e["name"], r)
        if e["group"] != "d":
            assert _sha(o) == e["sha256"], e["name"]


def test_routed_and_unrouted_frames_share_a_call(ctx, idx):
    """route auto: frames without a count take stage E, the others the block route, one refusal and one wrong count among
    them; the neighbours' outputs lie back to back"""
    by = {e["name"]: e for e in idx["cases"]}
    one = next(e for e in D.index()["frames"] if e["name"] == "a_text_3073_L1")
    picks = [(by["n_text_9000_L1"], None), (by["h_reach_first_byte"], None), (one, 0), (by["s_between_treeless"], None), (by["n_silesia_70001_L3"], 0),
             (by["r_earliest_wins"], None), (by["n_records_40000_L19"], None), (by["n_text_9000_L1"], 5)]
    frames = [B.frame_bytes(e) if "cap" in e else D.frame_bytes(e) for e, _ in picks]
    caps = [e.get("cap", e.get("content")) for e, _ in picks]
    counts = [e.get("nblocks", 1) if c is None else c for e, c in picks]
    res, outs = device_decode(ctx, frames, caps, counts, "auto")
    for (e, c), r, o in zip(picks, res, outs):
        if c == 5:
            assert r[0] == B.EHINT
            continue
        assert list(r) == e["sim"], (e["name"], r)
        if r[0] == 0:
            assert _sha(o) == e["sha256"], e["name"]


def test_a_session_reads_a_40_block_frame_from_the_host(idx):
    e = next(c for c in idx["cases"] if c["name"] == "n_text_40000_L3_cs")
    frame = B.frame_bytes(e)
    assert e["nblocks"] == 40
    for route in ("blocks", "auto", "frame"):
        z = A.Session(zstd_dec=A.QZ_DIR_DECOMPRESS)
        assert z.rc_setup == A.QZ_OK and z.zstd_decode_route(route) == A.QZ_OK
        small = D.frame_bytes(next(f for f in D.index()["frames"] if f["name"] == "a_text_3073_L1"))
        rc, used, out = z.decompress(small + frame + small, 3073 + 40000 + 3073)
        assert (rc, used) == (A.QZ_OK, 2 * len(small) + len(frame)), route
        assert _sha(out[3073:43073]) == e["sha256"] and out[:3073] == out[43073:] == S.make_input("text", 3073, 11), route
        assert z.zstd_decode_route(3) == A.QZ_PARAMS
        z.close()
    s = A.Session(lz4=True)
    assert s.zstd_decode_route("blocks") == A.QZ_PARAMS
    s.close()


def test_the_device_counts_what_the_host_counts(ctx, idx):
    entries = [B.frame_bytes(e) for e in idx["cases"]] + [D.frame_bytes(e) for e in D.index()["frames"] if e.get("cause") != "dictionary_id"]
    comp, segs, _ = D.layout(entries, [0] * len(entries))
    d_in = ctx.alloc(len(comp) + 64); d_in.upload(comp)
    got = ctx.zstd_count_blocks(d_in, [tuple(int(x) for x in s) for s in segs])
    d_in.free()
    assert [int(n) for n in got] == [B.walk_count(f) for f in entries]
    assert sum(1 for n in got if n > 1) > 20 and 0 in got


def _writer_frames(ctx, src, hw):
    d_src = ctx.alloc(len(src)); d_src.upload(src)
    d_dst = ctx.alloc(zstd_bound(len(src), hw) + 64)
    n, lens = ctx.zstd_compress_frames(d_src, len(src), d_dst, hw, 3, 1, dst_cap=zstd_bound(len(src), hw))
    out = d_dst.download(n).tobytes()
    d_src.free(); d_dst.free()
    frames, pos = [], 0
    for ln in lens:
        frames.append(out[pos:pos + int(ln)])
        pos += int(ln)
    return frames


def test_a_stitched_frame_of_this_writers_blocks(ctx):
    """the many-block frame of the test below where libzstd does not load, here at 9 blocks of 4 KB: always run"""
    src = datagen.gen_bytes("silesia", 9 * 4096 - 100, 7)
    frame = G.stitched(_writer_frames(ctx, src, 4096), window_byte=0x10)
    assert B.walk_count(frame) == 9
    for route in ("blocks", "frame"):
        res, outs = device_decode(ctx, [frame], [len(src)], [9], route)
        assert res[0] == (0, len(frame), len(src)) and outs[0] == src, route


def test_a_16_mib_frame_of_128_blocks_under_both_routes(ctx):
    n = 16 << 20
    src = datagen.gen_bytes("silesia", n, 20250523)
    if zstd_ref.available():
        frame = zstd_ref.compress(src, 3)
    else:
        frame = G.stitched(_writer_frames(ctx, src, 131072))
    assert B.walk_count(frame) == 128
    d_in = ctx.alloc(len(frame) + 64); d_in.upload(frame)
    d_out = ctx.alloc(n + 64)
    got = {}
    for route in ("blocks", "frame"):
        d_out.upload(bytes(4096), 0)
        res = ctx.zstd_decompress_frames(d_in, d_out, [(0, 0, len(frame), n)], nblocks=[128], route=route)
        assert (int(res[0]["status"]), int(res[0]["in_used"]), int(res[0]["out_len"])) == (0, len(frame), n), route
        got[route] = d_out.download(n).tobytes()
        assert got[route] == src, route
    assert int(ctx.zstd_count_blocks(d_in, [(0, 0, len(frame), n)])[0]) == 128
    d_in.free(); d_out.free()
