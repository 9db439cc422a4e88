"""The block route of the zstd decoder (qatzip_amd/csrc/qzk_zstdd_blocks.h: Plan, Entropy, Scan, Fix, Finish) on the CPU SIMT
emulator with the device layer's launch sequence and qzd_zstdd_host.h itself (tests/sim/sim_zstdd_blocks.cpp): the committed
multi-block frames of tests/golden/zstd_dec_blocks/ and of tests/golden/zstd_dec/ under route `blocks` and under route `frame`,
the strict reader tests/zstd_full_format.py as the model.  The emulator driver checks the guard bytes behind every out_cap,
around every round's scratch and behind the descriptors on every call (rc -3).  No GPU, no libzstd."""
import hashlib
import os
import subprocess

import pytest

import zstd_format
import zstd_full_format as ZF
import zstdd_blocks_sim as B
import zstdd_sim as D


def _sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def idx():
    return B.index()


def _run(cases, route):
    """all the cases in ONE call, outputs back to back -> per name (result, output)"""
    frames = [B.frame_bytes(e) for e in cases]
    res, outs = B.decode_frames(frames, [e["cap"] for e in cases], nblocks=[e["nblocks"] for e in cases], route=route)
    return {e["name"]: (r, o) for e, r, o in zip(cases, res, outs)}


@pytest.fixture(scope="module")
def by_blocks(idx):
    return _run(idx["cases"], "blocks")


@pytest.fixture(scope="module")
def by_frame(idx):
    return _run(idx["cases"], "frame")


def test_the_index_holds_what_it_promises(idx):
    cases = idx["cases"]
    good = [e for e in cases if e["sim"][0] == 0]
    tally = set(t for e in good for t in e["tally"])
    for t in (["lit:treeless", "block:raw", "block:rle", "nseq0", "checksum"] + ["%s:%s" % (a, m) for a in ("ll", "of", "ml") for m in ("predefined", "fse", "repeat", "rle")]
              + ["rep:%d:%s" % (c, l) for c in (1, 2, 3) for l in ("ll>0", "ll0")]):
        assert t in tally, t
    hand = set(t for e in good if e["group"] == "h" for t in e["tally"])
    assert not [t for t in ["rep:%d:%s" % (c, l) for c in (1, 2, 3) for l in ("ll>0", "ll0")] if t not in hand]
    assert all(e["blocks"] >= 2 and e["blocks"] == e["nblocks"] for e in good)
    assert any(e["blocks"] > 64 and e["blocks"] % B.group() for e in good)
    names = set(e["name"] for e in cases)
    for n in ("s_between_treeless", "s_between_repeat", "h_minus_chain", "h_repeat_each", "h_predefined_put_back_ll", "h_predefined_put_back_of",
              "h_predefined_put_back_ml", "h_no_trailing", "h_reach_first_byte", "r_symbolic_0",
              "r_repeat_nothing", "r_treeless_nothing", "r_earliest_wins", "r_eout_then_bits", "r_bits_then_eout", "r_distance_global", "r_cut_in_block_17",
              "r_content_one_more", "r_content_one_less", "r_checksum_missing"):
        assert n in names, n
    assert sum(1 for e in cases if e["sim"][0] == B.EHINT) == 3
    # a refusal is libzstd's refusal too, but for the ones listed with their reason
    lax = set(a["name"] for a in idx["libzstd_accepts"])
    for e in cases:
        if e["sim"][0] in (D.EDATA, D.ETRUNC, D.ECKSUM):
            assert (e["libzstd"] == "ok") == (e["name"] in lax) and e["reader"] != "ok", e["name"]
    assert max(e["size"] for e in cases) <= 32768 and sum(os.path.getsize(os.path.join(B.GOLDEN, f)) for f in os.listdir(B.GOLDEN)) < 300000


def test_route_blocks_gives_the_pinned_answers(idx, by_blocks):
    for e in idx["cases"]:
        r, out = by_blocks[e["name"]]
        assert list(r) == e["sim"], (e["name"], r)
        if r[0] == 0:
            assert r == (0, e["size"], e["cap"]) and _sha(out) == e["sha256"], e["name"]
    st = {e["name"]: by_blocks[e["name"]][0][0] for e in idx["cases"]}
    assert st["r_eout_then_bits"] == D.EOUT and st["r_bits_then_eout"] == D.EDATA and st["r_bits_alone"] == D.EDATA
    assert st["r_earliest_wins"] == D.EDATA and st["r_later_cut_alone"] == D.ETRUNC
    assert st["r_symbolic_0"] == st["r_symbolic_0_two_steps"] == st["r_distance_global"] == D.EDATA
    assert st["r_repeat_nothing"] == st["r_treeless_nothing"] == st["r_content_one_more"] == st["r_content_one_less"] == D.EDATA
    assert st["r_cut_in_block_17"] == st["r_checksum_missing"] == D.ETRUNC and st["r_checksum_wrong"] == D.ECKSUM
    assert st["r_out_cap_short"] == D.EOUT


def test_route_frame_gives_the_same_answers(idx, by_blocks, by_frame):
    for e in idx["cases"]:
        if e["sim"][0] == B.EHINT:
            assert by_frame[e["name"]][0] == (0, e["size"], e["cap"]), e["name"]        # (the count is not looked at)
        else:
            assert by_frame[e["name"]] == by_blocks[e["name"]], e["name"]


def test_the_strict_reader_agrees(idx, by_blocks):
    for e in idx["cases"]:
        r, out = by_blocks[e["name"]]
        try:
            info, end = ZF.decode_frame(B.frame_bytes(e))
        except zstd_format.FormatError:
            assert r[0] != 0, e["name"]
            continue
        if r[0] == 0:
            assert r == (0, end, len(info["data"])) and out == info["data"] and info["blocks"] == e["nblocks"], e["name"]
        else:
            assert r[0] in (D.EOUT, B.EHINT), e["name"]


def test_the_frames_of_zstd_dec_through_route_blocks():
    """every frame of tests/golden/zstd_dec/ whose blocks the host's walk counts - the one-block frames too: route `blocks`
    takes them - gives the answers its own index pins"""
    entries = [e for e in D.index()["frames"] if B.walk_count(D.frame_bytes(e))]
    assert sum(1 for e in entries if B.walk_count(D.frame_bytes(e)) > 1) >= 10 and any(e["group"] == "d" for e in entries)
    frames = [D.frame_bytes(e) for e in entries]
    info = {}
    res, outs = B.decode_frames(frames, [e["content"] for e in entries], info=info)
    assert info["routed"] == len(entries)
    for e, r, o in zip(entries, res, outs):
        assert list(r) == e["sim"], (e["name"], r)
        if e["group"] != "d":
            assert _sha(o) == e["sha256"], e["name"]


def test_routing_and_launches(idx):
    """auto routes frames of QZD_ZD_BLOCKS_MIN blocks and more, `blocks` every frame with a count, `frame` none; a call without
    a routed frame is stage E, stage X and the checksums, nothing else"""
    by = {e["name"]: e for e in idx["cases"]}
    m = B.blocks_min()
    assert m >= 2
    small = by["h_reach_first_byte"]                                 # 3 blocks
    big = by["n_text_9000_L1"]
    one = next(e for e in D.index()["frames"] if e["name"] == "a_text_3073_L1")
    assert small["nblocks"] == 3 and big["nblocks"] >= m and B.walk_count(D.frame_bytes(one)) == 1
    frames = [B.frame_bytes(small), B.frame_bytes(big), D.frame_bytes(one), B.frame_bytes(big)]
    caps = [small["cap"], big["cap"], one["content"], big["cap"]]
    want = [tuple(small["sim"]), tuple(big["sim"]), tuple(one["sim"]), tuple(big["sim"])]
    assert big["nblocks"] > m
    for route, counts, routed, launches in (("auto", None, 2 if m > 3 else 3, 8), ("blocks", None, 4, 7), ("frame", None, 0, 3),
                                            ("blocks", [0, 0, 0, 0], 0, 3), ("blocks", [0, big["nblocks"], 0, 0], 1, 8), ("auto", [3, m - 1, 1, m], 1, 8)):
        info = {}
        res, outs = B.decode_frames(frames, caps, nblocks=counts, route=route, info=info)
        if counts == [3, m - 1, 1, m]:                               # (the last frame has more blocks than m)
            assert (info["routed"], info["launches"]) == (sum(1 for c in counts if c >= m), 8) and res[3][0] == B.EHINT and res[:3] == want[:3]
            continue
        assert res == want and (info["routed"], info["launches"]) == (routed, launches), (route, counts, info)
        assert outs[1] == outs[3] and _sha(outs[1]) == big["sha256"]
    # NULL counts are the call without counts
    comp, segs, out_size = D.layout(frames, caps)
    rc, res, out, info = B.decode(comp, segs, out_size, None, "blocks")
    rc0, res0, out0, _ = D.decode(comp, segs, out_size)
    assert rc == rc0 == 0 and info["launches"] == 3 and out == out0 and res.tobytes() == res0.tobytes()


def test_groups_smaller_and_larger_than_a_wave_takes(idx):
    """frames of 3 blocks: 1, G - 1, G, G + 1 and 2 G + 1 of them are 3 .. 6 G + 3 descriptors over the waves' groups"""
    e = next(c for c in idx["cases"] if c["name"] == "h_reach_first_byte")
    fr = B.frame_bytes(e)
    G = B.group()
    for k in sorted(set([1, G - 1, G, G + 1, 2 * G + 1])):
        res, outs = B.decode_frames([fr] * k, [e["cap"]] * k)
        assert res == [tuple(e["sim"])] * k and all(_sha(o) == e["sha256"] for o in outs), k


def test_rounds_by_the_scratch_cap(idx):
    """a cap that holds one frame a round: the descriptors lie behind each round's scratch, the answers stay"""
    cases = [c for c in idx["cases"] if c["name"] in ("h_repeat_each", "h_minus_chain", "r_earliest_wins", "h_70_blocks")]
    frames = [B.frame_bytes(e) for e in cases]
    comp, segs, out_size = D.layout(frames, [e["cap"] for e in cases])
    rc, res, out, info = B.decode(comp, segs, out_size, [e["nblocks"] for e in cases], "blocks", scratch_cap=1)
    assert rc == 0 and info["rounds"] == len(cases) and info["routed"] == len(cases)
    assert [[int(r["status"]), int(r["in_used"]), int(r["out_len"])] for r in res] == [e["sim"] for e in cases]


def test_out_cap_one_below_and_above(idx):
    for name in ("h_repeat_each", "n_rand_5000_L1", "s_between_repeat", "h_no_trailing"):
        e = next(c for c in idx["cases"] if c["name"] == name)
        fr = B.frame_bytes(e)
        for cap, want in ((e["cap"] - 1, D.EOUT), (e["cap"] + 1, 0)):
            rb, _ = B.decode_frames([fr], [cap], gap=32)
            ra, _ = D.decode_frames([fr], [cap], gap=32)
            assert rb == ra and rb[0][0] == want, (name, cap, rb, ra)


def test_a_frame_without_content_size_at_every_cap(idx):
    """r_eout_then_bits has no Frame_Content_Size: whichever comes first in the stream - the record that passes out_cap, the
    block whose literals alone pass it, the end of the bit stream - both routes answer alike at every out_cap"""
    fr = B.frame_bytes(next(c for c in idx["cases"] if c["name"] == "r_eout_then_bits"))
    caps = list(range(0, 100))
    rb, _ = B.decode_frames([fr] * len(caps), caps, nblocks=[3] * len(caps))
    ra, _ = D.decode_frames([fr] * len(caps), caps)
    assert rb == ra and set(r[0] for r in rb) == {D.EOUT, D.EDATA}


def test_random_chains_of_table_modes_under_both_routes():
    """300 frames of 4 - 9 small blocks whose LL / OF / ML modes are drawn from Predefined, RLE_Mode and Repeat_Mode
    (tests/golden/gen_zstd_dec_blocks.py, random_chain; a fixed seed): a table is inherited over blocks that set, repeat or put
    back the others in every combination.  Both routes give what the strict reader gives"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_zstd_dec_blocks as G
    import numpy as np
    import zstd_sim
    text = zstd_sim.make_input("text", 600, 4)
    rng = np.random.Generator(np.random.PCG64(5))
    frames = [G.frame(G.random_chain(rng, 4 + i % 6, text)) for i in range(300)]
    datas = [ZF.decode_frame(f)[0]["data"] for f in frames]
    tally = set(t for f in frames for t in ZF.decode_frame(f)[0]["tally"])
    assert not [t for t in ["%s:%s" % (a, m) for a in ("ll", "of", "ml") for m in ("predefined", "rle", "repeat")] if t not in tally]
    want = [(0, len(f), len(d)) for f, d in zip(frames, datas)]
    for route in ("blocks", "frame"):
        res, outs = B.decode_frames(frames, [len(d) for d in datas], route=route)
        assert [i for i, (r, w) in enumerate(zip(res, want)) if r != w] == [] and outs == datas, route


def test_a_stitched_frame_of_this_writers_blocks():
    """what the GPU tests decode where libzstd does not load (tests/golden/gen_zstd_dec_blocks.py, stitched): the one-block
    frames of this project's writer as the blocks of one frame"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_zstd_dec_blocks as G
    import zstd_sim
    src = zstd_sim.make_input("silesia", 9 * 4096 - 100, 7)
    stream, lens = zstd_sim.compress(src, 4096, 3)
    frames, pos = [], 0
    for ln in lens:
        frames.append(stream[pos:pos + ln])
        pos += ln
    fr = G.stitched(frames, window_byte=0x10)
    assert B.walk_count(fr) == 9 and ZF.decode_frame(fr)[0]["data"] == src
    for route in ("blocks", "frame"):
        res, outs = B.decode_frames([fr], [len(src)], route=route)
        assert res[0] == (0, len(fr), len(src)) and outs[0] == src, route


def test_the_device_walk_counts_what_the_host_walk_counts(idx):
    entries = [(B.frame_bytes(e), e) for e in idx["cases"]] + [(D.frame_bytes(e), e) for e in D.index()["frames"]]
    frames = [f for f, _ in entries]
    got = B.count_blocks(frames)
    for (f, e), n in zip(entries, got):
        assert n == B.walk_count(f) or (n == 0 and e.get("cause") == "dictionary_id"), e["name"]
    assert sum(1 for n in got if n > 1) > 20 and 0 in got


def test_under_sanitizers(tmp_path, idx):
    """tests/sim/sim_zstdd_blocks.cpp as a program of its own (SIM_ZSTDDB_MAIN): the host plan and the emulator driver over
    the refusals and the hand-built frames under both routes, and one frame cut at every byte, every input in an allocation of
    exactly its size, built with -fsanitize=address,undefined.  A stand-alone program: nothing here is loaded into python."""
    exe = str(tmp_path / "sim_zstdd_blocks_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSIM_ZSTDDB_MAIN",
                           "-I", B.SIMDIR, "-Wno-unused-function", "-o", exe, B.SRC])
    files = sorted(set(os.path.join(B.GOLDEN, e["file"]) for e in idx["cases"] if e["size"] < 6000))
    assert len(files) >= 25
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
    # (h_70_blocks: more groups than one wave of 64 lanes takes; s_between_repeat: its first 4 KiB of cuts)
    for cut in (["h_repeat_each.zst"], ["h_70_blocks.zst"], ["s_between_repeat.zst", "0", str(CUT_MAX)]):
        r = subprocess.run([exe, "cut", os.path.join(B.GOLDEN, cut[0])] + cut[1:], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


CUT_MAX = 4096


def test_a_frame_cut_at_every_byte_under_both_routes(idx):
    """what the program above compares in C, here: the frame cut at every byte gives the same {status, in_used, out_len} and
    bytes under route `blocks` - the host walk's count, and where the walk fails the whole frame's - and under route `frame`"""
    for name in ("h_repeat_each", "h_70_blocks", "s_between_repeat"):
        e = next(c for c in idx["cases"] if c["name"] == name)
        fr = B.frame_bytes(e)
        last = min(len(fr), CUT_MAX)
        for first in range(0, last + 1, 512):                            # (calls of 512 cuts: every cut has the frame's out_cap)
            cuts = [fr[:n] for n in range(first, min(first + 512, last + 1))]
            caps = [e["cap"]] * len(cuts)
            ra, oa = D.decode_frames(cuts, caps)
            assert all(r == (D.ETRUNC, 0, 0) if len(c) < len(fr) else r == tuple(e["sim"]) for c, r in zip(cuts, ra)), name
            for counts in (None, [e["nblocks"]] * len(cuts)):
                rb, ob = B.decode_frames(cuts, caps, nblocks=counts)
                assert [first + n for n, (a, b) in enumerate(zip(ra, rb)) if a != b] == [] and oa == ob, name
