#!/usr/bin/env python3
"""Creates tests/golden/zstd_seq/index.json: what the zstd kernel (qatzip_amd/csrc/qzk_zstd.h) writes under seq_flags
(include/qzamd_zstd_seq.h) on the CPU SIMT emulator - the pin tests/test_sim_zstd_seq.py reproduces on the emulator and
tests/test_gpu_zstd_seq.py on the GPU.  Every pinned stream was decoded by the strict reader of whole frames
(tests/zstd_full_format.py) and by libzstd's ZSTD_decompress when this file was made.  Run it again only when the entropy
stage is changed on purpose; the output is committed.

index.json:
  cases   (kind, n, seed, hw_buff_sz, mini_match, flags): input SHA-256, stream length, stream SHA-256
  edges   per flags 1, 2, 3 and per hand-made frame of tests/zstd_seq_sim.py (EDGES, REP): the frame's length and SHA-256
  ratio   for the four corpora of tests/golden/zstd/index.json (262144 bytes, 64 KB chunks, mini_match 3) under flags 3: the
          total, its ratio to libzstd's ZSTD_compressSequences total recorded there (never this encoder's own output), and
          cap = ratio + 0.02, which the test asserts
  max_frame_excess   the largest (flags-3 frame - flags-0 frame of the same chunk) over all inputs of cases and ratio
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_ref  # noqa: E402
import zstd_seq_sim as Q  # noqa: E402
import zstd_sim  # noqa: E402

SEED = 11
KINDS = ("text", "records", "silesia", "lzmix", "runs", "mod200", "rand", "allA")
CASES = [(k, 70001, SEED, 65536, mm, 3) for k in KINDS for mm in (3, 4)] + [
    (k, 70001, SEED, 65536, 3, fl) for k in ("text", "records", "lzmix") for fl in (1, 2)] + [
    ("text", 3073, SEED, 1024, 3, 3), ("silesia", 300000, SEED, 4096, 3, 3), ("window", 131072, 5, 131072, 3, 3),
    ("far65535", 131072, 6, 131072, 4, 3), ("allA", 131072, SEED, 131072, 4, 3), ("merged", 73000, 8, 131072, 3, 3),
    ("records", 262144, SEED, 16384, 4, 3), ("silesia", 131072 + 777, SEED, 131072, 3, 1),
]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def main():
    assert zstd_ref.available(), "libzstd is needed for the second decode"
    old = zstd_sim.index()
    out = {"libzstd": zstd_ref.version(), "cases": [], "edges": {}, "ratio": []}
    excess = None
    for kind, n, seed, hw, mm, fl in CASES:
        src = zstd_sim.make_input(kind, n, seed)
        got, lens = Q.compress(src, hw, mm, fl)
        Q.read(got, src, hw)
        out["cases"].append({"kind": kind, "n": n, "seed": seed, "hw_buff_sz": hw, "mini_match": mm, "flags": fl, "in_sha": sha(src),
                             "out_len": len(got), "out_sha": sha(got)})
        if fl == 3:
            _, lens0 = zstd_sim.compress(src, hw, mm)
            excess = max([a - b for a, b in zip(lens, lens0)] + ([] if excess is None else [excess]))
    for fl in (1, 2, 3):
        names = sorted(Q.EDGES) + sorted(Q.REP)
        rc, stream, lens = Q.encode([Q.EDGES[k] if k in Q.EDGES else Q.REP[k] for k in names], fl)
        assert rc == 0
        pos, rec = 0, {}
        for k, ln in zip(names, lens):
            one = stream[pos:pos + ln]
            pos += ln
            fr = Q.EDGES[k] if k in Q.EDGES else Q.REP[k]
            zstd_ref.check(one, zstd_sim.rebuild(fr))
            rec[k] = [ln, sha(one)]
        out["edges"][str(fl)] = rec
    for r in old["ratio"]:
        src = zstd_sim.make_input(r["kind"], r["n"], r["seed"])
        assert sha(src) == r["in_sha"]
        got, lens = Q.compress(src, 65536, 3, 3)
        Q.read(got, src, 65536)
        _, lens0 = zstd_sim.compress(src, 65536, 3)
        excess = max([a - b for a, b in zip(lens, lens0)] + [excess])
        ratio = round(len(got) / r["libzstd_compress_sequences"], 4)
        out["ratio"].append({"kind": r["kind"], "n": r["n"], "seed": r["seed"], "in_sha": r["in_sha"], "zstd_seq_len": len(got),
                             "ratio": ratio, "cap": round(ratio + 0.02, 4)})
    out["max_frame_excess"] = excess
    os.makedirs(os.path.join(HERE, "zstd_seq"), exist_ok=True)
    with open(Q.INDEX, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for r in out["ratio"]:
        print(r)
    print("max_frame_excess", excess)


if __name__ == "__main__":
    main()
