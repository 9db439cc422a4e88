"""Kzp, the hash-chain lazy parse of zstd sessions (qatzip_amd/csrc/qzk_zstd_parse.h), decision by decision on the trap inputs
of tests/zstd_parse_traps.py without a GPU.  The authority is that module's serial model of the header's rules: on every trap
the CPU emulator's chain distances (P1), {length, distance} results (P2), records and literals (P3) equal the model's, and
the trap's check reads its aimed decision out of the model's answer.  The frames under all four sequence flags are read by the
strict reader and, where it loads, libzstd, which resolve the repeat codes on their own: their sequences and repeat tallies
are the model's.  Emulator builds with other -D constants follow the model with those constants and leave the default's
records on some trap; sixteen and more 1024-byte traps as the chunks of one call give the bytes of the traps one by one;
the stand-alone program of tests/sim/sim_zstd_parse.cpp runs the planted corners under -fsanitize=address,undefined.  The
-m gpu twin is tests/test_gpu_zstd_parse_traps.py."""
import functools
import hashlib
import json
import os
import subprocess

import pytest

import zstd_parse_sim as P
import zstd_parse_traps as T
import zstd_seq_sim as Q
import zstd_sim as S

HERE = os.path.dirname(os.path.abspath(__file__))
INDEX = os.path.join(HERE, "golden", "zstd_parse_traps", "index.json")
TRAPS = T.all_traps()
BY_NAME = {t.name: t for t in TRAPS}
MUTANTS = (("QZK_ZP_MINGAIN", "mingain", 9), ("QZK_ZP_MINGAIN", "mingain", 11), ("QZK_ZP_LAZY2", "lazy2", 63), ("QZK_ZP_LAZY2", "lazy2", 65),
           ("QZK_ZP_HSHIFT", "hshift", 1), ("QZK_ZP_HSHIFT", "hshift", 3))
SEARCH_SEEDS = range(100000, 100040)        # a short run of the state-machine search on fresh seeds


def sha(b):
    return hashlib.sha256(b).hexdigest()


def seq_sha(seqs):
    return sha(json.dumps([list(s) for s in seqs], separators=(",", ":")).encode())


@functools.lru_cache(maxsize=None)
def stages(name, hshift=2):
    """P1 and P2 of the model on a trap, once per head-table shift: (chain, res, their trace)"""
    t = BY_NAME[name]
    tr = T.Trace()
    tr.hit("p1.width.%d" % t.hw_buff_sz, 0)
    chain = T.p1_chain(t.data, t.hw_buff_sz, t.mini_match, hshift, tr)
    return chain, T.p2_search(t.data, chain, t.mini_match, t.depth, tr), tr


@functools.lru_cache(maxsize=None)
def answer(name, mingain=10, lazy2=64, hshift=2):
    """the model's (chain, res, seqs, literals, trace) on a trap; the default's is computed once and shared"""
    t = BY_NAME[name]
    chain, res, tr12 = stages(name, hshift)
    tr = T.Trace()
    tr.count.update(tr12.count)
    for k, v in tr12.where.items():
        tr.where[k] |= v
    seqs, lits = T.p3_lazy(t.data, res, t.mini_match, t.depth, mingain, lazy2, tr)
    return chain, res, seqs, lits, tr


@pytest.fixture(scope="module")
def index():
    with open(INDEX) as f:
        doc = json.load(f)
    return doc, {e["name"]: e for e in doc["traps"]}


def test_model_in_pieces_is_the_model():
    """answer() above runs the three stages on their own; on a handful of traps that is model()"""
    for t in TRAPS[::9]:
        chain, res, seqs, lits, tr = T.model(t.data, t.hw_buff_sz, t.mini_match, t.depth)
        a = answer(t.name)
        assert (chain, res, seqs, lits) == a[:4] and tr.count == a[4].count and dict(tr.where) == dict(a[4].where), t.name


# ---------------------------------------------------------------- per trap
@pytest.mark.parametrize("name", [t.name for t in TRAPS])
def test_emulator_equals_the_model_stage_by_stage(name):
    t = BY_NAME[name]
    chain, res, seqs, lits, tr = answer(name)
    echain, eres = P.search(t.data, t.hw_buff_sz, t.mini_match, t.depth)
    assert echain == chain, (name, "P1", [(p, a, b) for p, (a, b) in enumerate(zip(echain, chain)) if a != b][:5])
    assert eres == res, (name, "P2", [(p, a, b) for p, (a, b) in enumerate(zip(eres, res)) if a != b][:5])
    _, eseqs, elits = P.records(t.data, t.hw_buff_sz, t.mini_match, t.depth)
    assert eseqs == seqs, (name, "P3", t.aim, [(a, b) for a, b in zip(T.starts(eseqs), T.starts(seqs)) if a != b][:3])
    assert elits == lits, name
    assert t.check(seqs, tr), (name, t.aim, T.starts(seqs)[-8:])


@pytest.mark.parametrize("name", [t.name for t in TRAPS])
def test_frames_under_every_flag_hold_the_models_sequences(name, index):
    """flags 0 .. 3: the strict reader and libzstd decode the frame; the reader's sequences, repeat codes resolved by its own
    history, are the model's; with QZ_ZSTD_SEQ_REPEAT_OFFSETS the repeat codes it met are the ones predicted from the model's
    records, without it there is none.  (A chunk whose compressed block would not be smaller is a raw block under every
    flag: it holds no sequences, and the index says so.)"""
    t = BY_NAME[name]
    seqs = answer(name)[2]
    e = index[1][name]
    for flags in (0, 1, 2, 3):
        frame, lens = P.compress(t.data, t.hw_buff_sz, t.mini_match, flags, t.depth)
        f = Q.read(frame, t.data, t.hw_buff_sz)[0]
        reps = sorted(x for x in f["tally"] if x.startswith("rep:"))
        if "block:compressed" in f["tally"]:
            assert [tuple(s) for s in f["sequences"]] == seqs, (name, flags)
            assert reps == (Q.rep_tally(seqs) if flags & 2 else []), (name, flags)
        else:
            assert reps == [] and not f["sequences"], (name, flags)
        if flags in (0, 3):
            pin = e["frames"][str(flags)]
            assert (len(frame), sha(frame), "block:compressed" in f["tally"]) == (pin["len"], pin["sha256"], pin["compressed"]), (name, flags)
    assert Q.rep_tally(seqs) == e["rep"], name


# ---------------------------------------------------------------- the whole set
def test_every_label_has_a_trap_or_an_argument():
    """every label is asked for by the check of a trap (and every check holds on the model: the test above), or stands in
    UNREACHABLE, whose arguments the module's comment writes out; the module's docstring lists label by label which traps"""
    table = T.label_traps()
    silent = sorted(lab for lab, names in table.items() if not names)
    assert silent == sorted(T.UNREACHABLE), silent
    assert T.trap_table() in T.__doc__, "the docstring's list of labels and traps is out of date: paste zstd_parse_traps.trap_table()"
    src = open(os.path.join(HERE, "zstd_parse_traps.py")).read()
    for lab in T.UNREACHABLE:
        assert "# %s.  " % lab in src, lab
        assert not any(lab in answer(t.name)[4] for t in TRAPS), lab
    assert {t.family for t in TRAPS} == set(T.FAMILIES)
    assert {t.mini_match for t in TRAPS} == {3, 4} and {t.depth for t in TRAPS} >= set(T.DEPTHS) and {t.hw_buff_sz for t in TRAPS} == set(T.HWS)
    assert sum(1 for t in TRAPS if len(t.data) > 65536) <= 3 and all(len(t.data) <= 8192 for t in TRAPS if t.depth == 256)
    assert len([t for t in TRAPS if len(t.data) == t.hw_buff_sz == 1024]) >= 16


def test_index_is_in_step(index):
    doc, idx = index
    assert [t.name for t in TRAPS] == list(idx) and doc["labels"] == list(T.LABELS)
    for t in TRAPS:
        e = idx[t.name]
        assert (len(t.data), t.hw_buff_sz, t.mini_match, t.depth, t.family, sha(t.data)) == \
            (e["n"], e["hw_buff_sz"], e["mini_match"], e["depth"], e["family"], e["input_sha256"]), t.name
        seqs, tr = answer(t.name)[2], answer(t.name)[4]
        assert (seq_sha(seqs), len(seqs)) == (e["seq_sha256"], e["nseq"]), t.name
        assert sorted(doc["labels"][i] for i in e["labels"]) == tr.labels(), t.name


# ---------------------------------------------------------------- mutants by macro
def test_builds_with_other_constants_follow_the_model_and_leave_the_default(tmp_path):
    """the emulator built with QZK_ZP_MINGAIN 9 / 11, QZK_ZP_LAZY2 63 / 65, QZK_ZP_HSHIFT 1 / 3: on every trap its records
    are model(...)'s with that constant, and on some trap they are not the default's - the traps tell the constants apart
    and the model follows the rules, not the pins"""
    procs = []
    for macro, kw, v in MUTANTS:
        so = str(tmp_path / ("libzp_%s_%d.so" % (kw, v)))
        procs.append((so, subprocess.Popen(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D%s=%d" % (macro, v), "-I", S.SIMDIR, "-Wno-unused-function", "-o", so, P.SRC])))
    for (macro, kw, v), (so, proc) in zip(MUTANTS, procs):
        assert proc.wait() == 0, macro
        lib = P.load(so)
        differs = []
        for t in TRAPS:
            if not t.data:
                continue
            _, seqs, lits = P.records(t.data, t.hw_buff_sz, t.mini_match, t.depth, lib=lib)
            want = answer(t.name, **{kw: v})
            assert (seqs, lits) == (want[2], want[3]), (macro, v, t.name)
            if kw == "hshift":
                assert P.search(t.data, t.hw_buff_sz, t.mini_match, t.depth, lib=lib) == (want[0], want[1]), (macro, v, t.name)
            if seqs != answer(t.name)[2]:
                differs.append(t.name)
        print("%s=%d: records differ from the default on" % (macro, v), differs)
        assert differs, (macro, v)


# ---------------------------------------------------------------- chunks of one call
def test_traps_as_the_chunks_of_one_call():
    """the 1024-byte traps of one mini_match and depth, concatenated: one call at hw_buff_sz 1024, in one round of the host
    plan and in rounds of one chunk, gives the frames of the traps one by one"""
    group = T.independent_traps()
    assert len(group) >= 16
    hw, mm, depth = T.CI
    alone = [P.compress(t.data, hw, mm, 3, depth)[0] for t in group]
    cat = b"".join(t.data for t in group)
    for cap in (0, 1):
        got, lens = P.compress(cat, hw, mm, 3, depth, round_cap=cap)
        assert lens == [len(a) for a in alone] and got == b"".join(alone), cap


def test_a_short_run_of_the_search_against_the_emulator():
    """fresh seeds of the state-machine search: model and emulator agree at all three stages on every input visited, and no
    label of UNREACHABLE shows"""
    seen = set()
    for seed in SEARCH_SEEDS:
        n = T.SM_SIZES[seed & 1]
        src = T.sm_input(seed, n)
        mm, depth = T.SM_MODES[seed % len(T.SM_MODES)]
        chain, res, seqs, lits, tr = T.model(src, T.K1, mm, depth)
        assert (chain, res) == P.search(src, T.K1, mm, depth), (seed, n, mm, depth)
        assert (seqs, lits) == P.records(src, T.K1, mm, depth)[1:], (seed, n, mm, depth)
        seen |= set(tr.labels())
    assert not seen & set(T.UNREACHABLE) and len(seen) >= 40, sorted(seen)
