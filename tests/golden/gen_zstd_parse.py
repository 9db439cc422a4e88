#!/usr/bin/env python3
"""Creates tests/golden/zstd_parse/index.json: what a zstd session writes under a parse depth (include/qzamd_zstd_parse.h,
qatzip_amd/csrc/qzk_zstd_parse.h) on the CPU SIMT emulator - the pin tests/test_sim_zstd_parse.py reproduces on the emulator
and tests/test_gpu_zstd_parse.py on the GPU.  Every pinned stream was decoded by the strict reader of whole frames
(tests/zstd_full_format.py) and by libzstd's ZSTD_decompress when this file was made.  Run it again only when the parse is
changed on purpose; the output is committed.

index.json:
  edges   per case of zstd_parse_sim.edge_cases() (flags 3): hw_buff_sz, mini_match, depth, input SHA-256, stream length,
          stream SHA-256
  cases   the eight kinds of gen_zstd_seq.py at 70001 bytes, 64 KB chunks, mini_match 3, depth 16, flags 3: the same
  ratio   for the four corpora of tests/golden/zstd/index.json (262144 bytes, 64 KB chunks, mini_match 3, flags 3): this
          writer's total per depth 4, 16, 64; the totals of libzstd's ZSTD_compress on each 64 KB chunk alone at levels 1,
          3 and 9 (from the library, never from this code); per depth the ratio to level 3 and cap = ratio + 0.02, which
          the test asserts
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_parse_sim as P  # noqa: E402
import zstd_ref  # noqa: E402
import zstd_seq_sim as Q  # noqa: E402
import zstd_sim  # noqa: E402

SEED = 11


def sha(b):
    return hashlib.sha256(b).hexdigest()


def main():
    assert zstd_ref.available(), "libzstd is needed for the second decode and the yardsticks"
    old = zstd_sim.index()
    default = {r["kind"]: r["zstd_seq_len"] for r in Q.index()["ratio"]}
    out = {"libzstd": zstd_ref.version(), "edges": {}, "cases": [], "ratio": []}
    for name, (src, hw, mm, depth) in P.edge_cases().items():
        got, lens = P.compress(src, hw, mm, 3, depth)
        Q.read(got, src, hw)
        out["edges"][name] = {"hw_buff_sz": hw, "mini_match": mm, "depth": depth, "in_sha": sha(src), "out_len": len(got), "out_sha": sha(got)}
    for kind in P.KINDS:
        src = zstd_sim.make_input(kind, 70001, SEED)
        got, lens = P.compress(src, 65536, 3, 3, 16)
        Q.read(got, src, 65536)
        out["cases"].append({"kind": kind, "n": 70001, "seed": SEED, "hw_buff_sz": 65536, "mini_match": 3, "depth": 16, "flags": 3,
                             "in_sha": sha(src), "out_len": len(got), "out_sha": sha(got)})
    for r in old["ratio"]:
        src = zstd_sim.make_input(r["kind"], r["n"], r["seed"])
        assert sha(src) == r["in_sha"]
        lib = {str(lv): sum(len(zstd_ref.compress(src[i:i + 65536], lv)) for i in range(0, len(src), 65536)) for lv in P.LIBZSTD_LEVELS}
        rec = {"kind": r["kind"], "n": r["n"], "seed": r["seed"], "in_sha": r["in_sha"], "default_flags3": default[r["kind"]],
               "libzstd_compress": lib, "depths": {}}
        for depth in P.RATIO_DEPTHS:
            got, _ = P.compress(src, 65536, 3, 3, depth)
            Q.read(got, src, 65536)
            ratio = round(len(got) / lib["3"], 4)
            rec["depths"][str(depth)] = {"len": len(got), "ratio": ratio, "cap": round(ratio + 0.02, 4)}
        out["ratio"].append(rec)
        print(r["kind"], "default", default[r["kind"]], "libzstd", lib, {d: v["len"] for d, v in rec["depths"].items()},
              "depth 64 against level 1: %s" % ("at or below" if rec["depths"]["64"]["len"] <= lib["1"] else "ABOVE"))
    os.makedirs(os.path.join(HERE, "zstd_parse"), exist_ok=True)
    with open(P.INDEX, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
