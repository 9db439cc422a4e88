"""The block route of the zstd decoder (qatzip_amd/csrc/qzk_zstdd_blocks.h, qzd_zstdd_host.h) on the CPU SIMT emulator against
corrupted many-block frames: every bit of every frame of tests/golden/zstd_dec_blocks/ up to 1536 bytes flipped - the good
ones and the refusals with status -1 to -4 - bounded positions of the ten larger ones, and six substitutions at every byte of
a header field (tests/zstdd_blocks_mutate.py has the bases, the positions and their rule).  include/qzamd_zstd_blocks.h: "a
frame that takes it with a wrong count answers QZD_ZSTD_EHINT; every other answer is that of qzd_zstd_decompress_frames".
Per mutant, in calls with a good frame - three of many blocks, one of one - at the front, at the back and at every multiple
of QZK_ZD_G, each of which must still decode to its SHA:

    a  route `blocks` with the host walk's count, which is what qzDecompress does: {status, in_used, out_len} and the bytes are
       stage E's on the same call; rules 2 and 3 of tests/test_sim_zstdd_corrupt.py against the strict reader and libzstd hold,
       and the classes of rule 4 are among the committed ones of tests/golden/zstd_dec_corrupt/index.json;
    b  route `blocks` with the base's count, the stale hint: EHINT with in_used == out_len == 0 exactly where the document's
       sentence owes it (zstdd_blocks_mutate.owes_ehint: by the block headers alone), and then the host walk's count is another;
       otherwise stage E's answer and bytes; where the host walk gives the base's count, (a)'s;
    c  route `auto` with the host walk's count, on the frames flipped whole: (a)'s;
    d  the emulator driver's guard bytes - behind every out_cap, around every round's scratch, behind the descriptors - are
       untouched on every call; the frames the driver routed are the ones with a count.

ETRUNC cannot be the answer of a frame the host walk counts: the walk succeeds only where every block and the checksum lie
inside the input (no routed mutant of 56,675 has it).  So every status occurs under (a), every one but ETRUNC on a routed
mutant there, and ETRUNC on a routed mutant under (b), where the stale count routes a cut frame.

No mutant is skipped or sampled: the total is derived from the bases and asserted.  75,450 mutants of 38 bases, each decoded
three or four times, in jobs over up to eight processes: 220 s of wall time on the eight cores it was written on (29 minutes
of CPU, three quarters of them the 30,578 mutants of the ten larger frames), both references included; the sample under the
sanitizers takes another 70 s.  No GPU."""
import collections

import pytest

import zstdd_blocks_mutate as X
import zstdd_blocks_sim as B
import zstdd_mutate as M
import zstdd_sim as D


@pytest.fixture(scope="module")
def sweep():
    return X.run()


def test_the_bases_and_their_positions():
    bases = X.bases()
    cases = B.index()["cases"]
    assert [b.name for b in bases if b.name.startswith("r_count")] == [] and len(bases) == len(cases) - 3 == 38
    assert set(b.name for b in bases) == set(e["name"] for e in cases if e["sim"][0] in (0, -1, -2, -3, -4))
    assert all(b.exhaustive == (len(b.frame) <= M.EXHAUSTIVE_MAX) and (not b.exhaustive or len(b.flip_positions()) == len(b.frame)) for b in bases)
    assert [b.exhaustive for b in bases] == sorted((b.exhaustive for b in bases), reverse=True)
    by = {b.name: b for b in bases}
    assert by["h_70_blocks"].exhaustive and sorted(by["r_cut_in_block_17"].kept()) == [0, 1, 17]
    assert sorted(by["s_between_treeless"].kept()) == sorted(by["s_between_repeat"].kept()) == [4, 5, 60]
    for b in bases:
        if b.exhaustive:
            continue
        flips, blocks = set(b.flip_positions()), b.blocks()
        assert len(blocks) == (B.walk_count(b.frame) or 18), b.name             # (r_cut_in_block_17: the walk fails in block 17)
        assert all(p in flips for p, _ in blocks) and all(p in flips for name, a, e in b.sections if name in ("frame_header", "checksum") for p in range(a, e))
        for k in b.kept():
            assert all(p in flips for p in range(max(blocks[k][0], blocks[k][1] - M.SIDE), blocks[k][1])), (b.name, k)
            assert all(p in flips for p in range(blocks[k][0], min(blocks[k][1], blocks[k][0] + 3 + M.BLOCK_HEAD))), (b.name, k)
        assert set(b.field_positions()) <= flips


def test_no_mutant_is_skipped(sweep):
    bases = X.bases()
    expected = sum(8 * len(b.flip_positions()) + M.SUBSTITUTES * len(b.field_positions()) for b in bases)
    assert sweep["total"] == sweep["expected"] == expected >= 70000
    assert all(sweep["per_base"][b.name] == b.count() for b in bases)
    assert [r[:3] for r in sweep["records"]] == [(b.name, p, v) for b in bases for p, v in b.recipes()]
    print("\n%d mutants of %d bases in %.0f s" % (sweep["total"], len(bases), sweep["seconds"]))


def test_both_counts_stage_e_the_readers_the_guards_and_the_neighbours(sweep):
    """(a) to (d): every violation is listed"""
    v = sweep["violations"]
    assert not v, "%d violations, the first:\n%s" % (len(v), "\n".join(v[:40]))


def test_the_sweep_takes_the_block_route(sweep):
    """a condition, not a measurement: a sweep that falls back to stage E tests nothing"""
    rec = sweep["records"]
    routed = [r for r in rec if r[3]]
    print("\n%d of %d mutants routed under (a); under (a): %s; under (b): %s" % (
        len(routed), len(rec), sorted(collections.Counter(r[4][0] for r in rec).items()), sorted(collections.Counter(r[5][0] for r in rec).items())))
    assert 2 * len(routed) >= len(rec)
    assert set(r[4][0] for r in rec) == set(M.STATUSES) | {0}
    assert set(r[4][0] for r in routed) == (set(M.STATUSES) | {0}) - {D.ETRUNC}
    under_b = set(r[5][0] for r in rec)
    assert B.EHINT in under_b and D.ETRUNC in under_b
    assert all(r[5][1:] == (0, 0) and r[3] != X._base(r[0]).nblocks for r in rec if r[5][0] == B.EHINT)
    assert sum(1 for r in rec if r[8] > 0) > 10000 and sum(1 for r in rec if r[9] and r[3]) > 1000


def test_the_classes_of_strictness_are_among_the_committed(sweep):
    """rule 4: the block route refuses nothing of libzstd's that stage E does not"""
    if not sweep["with_lib"]:
        print("libzstd does not load here: rule 3 and the classes stand unchecked")
        return
    print("\nrefused here, accepted by libzstd, per class:")
    for c, n in sorted(sweep["classes"].items()):
        print("%7d  %s" % (n, c))
    assert not [c for c in sweep["classes"] if c not in M.hand_index()["classes"]]


def test_a_frame_a_round(sweep):
    """scratch_cap = 1: the descriptors lie behind each round's scratch; the first mutants of the frames flipped whole"""
    done, violations = X.scratch_slice(sweep)
    assert done == X.SCRATCH_SLICE and not violations, violations[:20]


def test_the_gpu_sample_is_the_sweeps(sweep):
    """the sample tests/test_gpu_zstd_dec_blocks_corrupt.py runs is what this sweep gives: nothing reaches the GPU whose answer
    was not obtained here, and none of these answers is a fault"""
    if not sweep["with_lib"]:
        return
    lines = X.gpu_sample(sweep)
    assert lines == X.sample()
    rows = X.parse_sample(lines)
    assert 1000 <= sum(1 for r in rows if r[6]) <= 5000 and any(not r[6] and r[4][0] == B.EHINT for r in rows)


def test_the_sample_under_sanitizers(tmp_path):
    """tests/sim/sim_zstdd_blocks.cpp as a program of its own (SIM_ZSTDDB_MAIN, `recipe` mode) over the committed sample under
    both routes, built with -fsanitize=address,undefined.  A stand-alone program: nothing here is loaded into python."""
    lines = X.sample()
    rows = X.parse_sample(lines)
    assert X.sanitizer_run(str(tmp_path), lines) == len(rows) + sum(1 for r in rows if r[6])
