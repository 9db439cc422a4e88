"""The zstd decode kernels (qatzip_amd/csrc/qzk_zstdd.h) on the CPU SIMT emulator against corrupted and hand-built frames:
every bit of every small committed frame and of the hand-built frames of tests/golden/zstd_dec_corrupt/ flipped, the header
and section-boundary bytes of three larger frames flipped, and six substitutions at every byte of a header field
(tests/zstdd_mutate.py has the order).  Per mutant, with out_cap the base's content plus 64:

    1  the emulator driver's guard bytes are untouched;
    2  the decoder accepts exactly when the strict reader tests/zstd_full_format.py does, with its bytes, in_used and out_len;
       a refusal has one of the five documented codes and in_used == out_len == 0 (a checksum mismatch keeps the frame's, as
       include/qzamd_device.h says);
    3  where libzstd loads, the decoder accepts only what ZSTD_decompress accepts, with the same bytes;
    4  what the decoder refuses and libzstd accepts falls into the committed list of classes - the strict reader's message
       without its numbers; a new class, or a vanished one, fails;
    5  mutants go in calls with a good frame at the front, at the back and at every multiple of QZK_ZD_G; each must still
       decode to its SHA.

No mutant is skipped or sampled: the total is derived from the bases' sizes and asserted.  The sweep is 110,146 mutants in
jobs over up to eight processes: 185 s of wall time on the eight cores it was written on (24 minutes of CPU, four fifths of
them the 7,636 mutants of the 300,000-byte frame, each a whole decode here and in the strict reader), both references
included.  No GPU."""
import pytest

import zstd_format
import zstd_full_format as ZF
import zstd_ref
import zstdd_mutate as M
import zstdd_sim as D


@pytest.fixture(scope="module")
def hand():
    return M.hand_index()


@pytest.fixture(scope="module")
def sweep():
    return M.run()


def test_the_hand_built_index_holds_every_feature_it_promises(hand):
    union = set(t for e in hand["frames"] for t in e.get("tally", []))
    required = (["hufbits:2", "hufbits:3", "hufbits:4", "hufbits:8", "weights:direct128", "wlog:5", "wlog:6", "lit:stream4:0",
                 "lit:stream4:1", "lit:1stream:1", "lit:treeless<raw<huffman", "tablelog:ll:5", "tablelog:ll:9", "tablelog:ml:5", "tablelog:ml:9", "tablelog:of:5",
                 "tablelog:of:8", "ncount:lessthan1", "ncount:zrun:1", "ncount:zrun:3", "ncount:zrun:4", "ncount:zrun:7", "ncount:lastbits:8",
                 "ncount:lastbits:1", "repeat<nseq0<rle", "repeat<nseq0<predefined", "repeat<nseq0<fse", "block:raw:empty-last",
                 "block:rle:1", "block:rle:max", "block:compressed:max", "block:at-window", "window:mantissa", "content:255",
                 "content:256", "content:65791", "content:65792", "seq0:ll1:ml3:off1", "offset:all-produced"])
    assert not [t for t in required if t not in union]
    refusals = {e["name"]: e for e in hand["frames"] if e["kind"] == "refusal"}
    for name in ("compressed_max_plus_1", "window_block_plus_1", "offset_all_produced_plus_1", "repeat3_ll0_rep1_later_block",
                 "huffman_no_weight_1_w3", "huffman_no_weight_1_w5", "huffman_no_weight_1_w9"):
        assert name in refusals, name
    # what libzstd 1.4.8 did with the refusals, as recorded: its one-shot path compares no block with the window or with
    # Block_Maximum_Size and turns a repeat offset of 0 into 1 - the decoder refuses all three, the permitted direction
    assert refusals["window_block_plus_1"]["libzstd"] == "ok" and refusals["window_block_plus_1"]["sim"] == [D.EDATA, 0, 0]
    assert all(e["libzstd"] == "ok" for e in hand["frames"] if e["kind"] == "ok")
    assert all(refusals["huffman_no_weight_1_w%d" % w]["libzstd"] != "ok" for w in (3, 5, 9))
    assert max(e["size"] for e in hand["frames"]) <= 1536


def test_every_hand_built_frame_against_the_strict_reader_libzstd_and_its_pin(hand):
    """rules 1 to 3 on the frames as they are, in one call with the refusals between the good ones"""
    entries = hand["frames"]
    frames = [M.hand_bytes(e) for e in entries]
    res, outs = D.decode_frames(frames, [e["content"] + 64 for e in entries])
    for e, f, r, o in zip(entries, frames, res, outs):
        assert list(r) == e["sim"], (e["name"], r)
        try:
            info, end = ZF.decode_frame(f)
        except zstd_format.FormatError as ex:
            assert e["kind"] == "refusal" and r[0] in M.STATUSES and r[1:] == (0, 0) and str(ex) == e["reader"], (e["name"], r, str(ex))
            continue
        assert e["kind"] == "ok" and r == (0, end, len(info["data"])) and o == info["data"], (e["name"], r)
        assert M.sha(o) == e["sha256"] and info["tally"] == e["tally"], e["name"]
        if zstd_ref.available():
            assert zstd_ref.decompress(f, e["content"] + 64) == o, e["name"]
    if zstd_ref.available():
        for e, f in zip(entries, frames):
            assert M.libzstd(f, e["content"] + 64)[0] == e["libzstd"], e["name"]


def test_sections_are_additive_and_cover_the_frame():
    for e in D.index()["frames"]:
        if e["group"] == "d":
            continue
        info, end = ZF.decode_frame(D.frame_bytes(e))
        sec = info["sections"]
        assert sec[0][0] in ("frame_header",) and sec[0][1] == 0
        assert all(a <= b for _, a, b in sec) and [s[1] for s in sec[1:]] == [s[2] for s in sec[:-1]] and sec[-1][2] == end, e["name"]


def test_no_mutant_is_skipped(sweep):
    """every mutant generated is counted: 8 flips per byte in range and 6 substitutions per header-field byte"""
    bases = M.bases()
    expected = sum(8 * len(b.flip_positions()) + 6 * len(b.field_positions()) for b in bases)
    assert sweep["total"] == sweep["expected"] == expected >= 40000
    assert all(sweep["per_base"][b.name] == b.count() for b in bases)
    whole = [b for b in bases if b.exhaustive]
    assert all(len(b.flip_positions()) == len(b.frame) for b in whole)
    assert set(b.name for b in bases if not b.exhaustive) == set(M.LARGE)
    print("\n%d mutants of %d bases in %.0f s" % (sweep["total"], len(bases), sweep["seconds"]))


def test_guards_reader_libzstd_and_neighbours(sweep):
    """rules 1, 2, 3 and 5: every violation is listed"""
    v = sweep["violations"]
    assert not v, "%d violations, the first:\n%s" % (len(v), "\n".join(v[:40]))


def test_the_finding_is_refused(sweep):
    """c_edge_two with its one direct weight changed from 1 to 3, 5 or 9: two one-bit codes and no symbol of weight 1, which
    libzstd's HUF_readStats refuses"""
    got = {(p, v): r for name, p, v, r, _, _ in sweep["records"] if name == "c_edge_two" and p == 17 and v in (3, 5, 9)}
    assert len(got) == 3 and all(r == (D.EDATA, 0, 0) for r in got.values()), got


def test_the_classes_of_strictness_are_the_committed_list(sweep, hand):
    """rule 4"""
    if not sweep["with_lib"]:
        print("libzstd does not load here: the committed list stands unchecked")
        return
    print("\nrefused here, accepted by libzstd, per class:")
    for c, n in sorted(sweep["classes"].items()):
        print("%7d  %s" % (n, c))
    assert sorted(sweep["classes"]) == hand["classes"]


def test_the_gpu_sample_is_the_sweeps(sweep, hand):
    """the sample tests/test_gpu_zstdd_corrupt.py runs is what this sweep gives: nothing reaches the GPU whose answer was
    not obtained here"""
    if not sweep["with_lib"]:
        return
    assert M.gpu_sample(sweep) == hand["sample"]


def test_the_sample_under_sanitizers(tmp_path, hand):
    """tests/sim/sim_zstdd.cpp as a program of its own (SIM_ZSTDD_MAIN, `recipe` mode) over the hand-built frames and the
    committed sample, built with -fsanitize=address,undefined.  A stand-alone program: nothing here is loaded into python."""
    ran = M.sanitizer_run(str(tmp_path), hand["sample"])
    assert ran == len(hand["sample"]) + len(hand["frames"])
