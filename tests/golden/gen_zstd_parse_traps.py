#!/usr/bin/env python3
"""Writes tests/golden/zstd_parse_traps/index.json: per trap of tests/zstd_parse_traps.py the input's SHA-256, the SHA-256 of
the serial model's sequence list, the labels its trace fired, the repeat codes it predicts (in the form of
zstd_seq_sim.rep_tally) and the frame's length and SHA-256 under sequence flags 0 and 3.

Order of trust: the model (zstd_parse_traps.model, written from the comment of qatzip_amd/csrc/qzk_zstd_parse.h) is held equal
to the CPU emulator of the kernels at all three stages - P1's chain distances, P2's {length, distance}, P3's records and
literals - and the trap's check must hold on the model's answer.  Only then are the frames taken from the emulator, each
after the strict reader (and libzstd, where it loads: "libzstd" in the index says whether it did) decoded it to the input
and returned the model's sequences with the repeat codes resolved.  Nothing in the index comes from the kernels before the
model agreed.  Inputs are rebuilt from zstd_parse_traps.py, never stored.

  --search [count]   the seeded search over sm_input(): per label of P3 the smallest input (size, seed, mini_match, depth)
                     whose trace holds it, printed as SM_SEEDS, and the labels it never saw - those of UNREACHABLE must be
                     among them.  Every 50th input it visits is also held against the emulator.
"""
import hashlib
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_parse_sim as P  # noqa: E402
import zstd_parse_traps as T  # noqa: E402
import zstd_ref  # noqa: E402
import zstd_seq_sim as Q  # noqa: E402

OUT = os.path.join(HERE, "zstd_parse_traps", "index.json")
LABEL_NO = {name: i for i, name in enumerate(T.LABELS)}


def sha(b):
    return hashlib.sha256(b).hexdigest()


def seq_sha(seqs):
    return sha(json.dumps([list(s) for s in seqs], separators=(",", ":")).encode())


def hold_equal(t):
    """the model against the emulator on one trap, all three stages -> the model's answer"""
    chain, res, seqs, lits, tr = T.model(t.data, t.hw_buff_sz, t.mini_match, t.depth)
    if t.data:
        echain, eres = P.search(t.data, t.hw_buff_sz, t.mini_match, t.depth)
        assert chain == echain, ("P1: the model's chain differs from the emulator's", t.name)
        assert res == eres, ("P2: the model's results differ from the emulator's", t.name)
        _, eseqs, elits = P.records(t.data, t.hw_buff_sz, t.mini_match, t.depth)
        assert (seqs, lits) == (eseqs, elits), ("P3: the model's records differ from the emulator's", t.name)
    return seqs, lits, tr


def _search_job(arg):
    n, seed = arg
    src = T.sm_input(seed, n)
    out = []
    for mm, depth in T.SM_MODES:
        chain, res, seqs, lits, tr = T.model(src, T.K1, mm, depth)
        if seed % 50 == 0:
            assert (chain, res) == P.search(src, T.K1, mm, depth) and (seqs, lits) == P.records(src, T.K1, mm, depth)[1:], (n, seed, mm, depth)
        out.append((n, seed, mm, depth, tr.labels()))
    return out


def search(count):
    best = {}
    with multiprocessing.Pool(min(16, len(os.sched_getaffinity(0)))) as pool:
        for n in T.SM_SIZES:
            for runs in pool.imap(_search_job, [(n, seed) for seed in range(count)], chunksize=20):
                for n_, seed, mm, depth, labels in runs:
                    for lab in labels:
                        best.setdefault(lab, (n_, seed, mm, depth))
    p3 = list(T.LABELS)[list(T.LABELS).index("stored.refused_9"):]
    print("SM_SEEDS = {")
    for lab in p3:
        if lab in best:
            print('    "%s": %r,' % (lab, best[lab]))
    print("}")
    never = [lab for lab in T.LABELS if lab not in best and not lab.startswith("p1.width")]
    print("never seen in %d inputs per size:" % count, never)
    assert all(lab in never for lab in T.UNREACHABLE)


def build():
    traps, census = [], {lab: 0 for lab in T.LABELS}
    libzstd = zstd_ref.available() if hasattr(zstd_ref, "available") else None
    for t in T.all_traps():
        seqs, lits, tr = hold_equal(t)
        assert t.check(seqs, tr), ("the check fails on the model: the trap tests nothing", t.name, t.aim)
        rec = {"name": t.name, "family": t.family, "n": len(t.data), "hw_buff_sz": t.hw_buff_sz, "mini_match": t.mini_match, "depth": t.depth,
               "input_sha256": sha(t.data), "seq_sha256": seq_sha(seqs), "nseq": len(seqs), "labels": sorted(LABEL_NO[x] for x in tr.labels()),
               "rep": Q.rep_tally(seqs), "frames": {}}
        for flags in (0, 3):
            frame, lens = P.compress(t.data, t.hw_buff_sz, t.mini_match, flags, t.depth)
            f = Q.read(frame, t.data, t.hw_buff_sz)[0]                  # the strict reader and, where it loads, libzstd
            if "block:compressed" in f["tally"]:
                assert [tuple(s) for s in f["sequences"]] == seqs, ("the reader's sequences differ from the model's", t.name, flags)
            rec["frames"][str(flags)] = {"len": len(frame), "sha256": sha(frame), "compressed": "block:compressed" in f["tally"]}
        for lab in ASKED[t.name]:
            census[lab] += 1
        traps.append(rec)
    print(T.trap_table())
    silent = [lab for lab in T.LABELS if not census[lab]]
    assert sorted(silent) == sorted(T.UNREACHABLE), silent
    doc = {"model": "tests/zstd_parse_traps.py model(), held equal to the emulator at P1, P2 and P3 on every trap", "libzstd": libzstd,
           "labels": list(T.LABELS), "census": census, "traps": traps}
    return json.dumps(doc, separators=(",", ":")).replace('{"name"', '\n{"name"') + "\n"


if __name__ == "__main__":
    if "--search" in sys.argv:
        i = sys.argv.index("--search")
        search(int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 20000)
    else:
        T.all_traps()
        ASKED = T.ASKS
        doc = build()
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(doc)
        print("wrote", OUT)
