#!/usr/bin/env python3
"""Creates tests/golden/lz4s/index.json: what the LZ4s kernel (qatzip_amd/csrc/qzk_lz4s.h) writes on the CPU SIMT emulator
for a fixed list of inputs - the pin tests/test_sim_lz4s.py reproduces on the emulator and tests/test_gpu_lz4s.py on the GPU
(the two builds must give the same bytes).  Run it again only when the parse is changed on purpose; the output is committed.

index.json:
  cases   (kind, n, seed, hw_buff_sz, mini_match): input SHA-256, stream length, stream SHA-256
  ratio   for the corpora of the ratio gate (262144 bytes, 64 KB chunks, mini_match 3): the sum of liblz4 1.9.3's level-1
          block bodies (LZ4_compress_default per chunk) - recorded here, where the library is installed, so that the gate
          does not need it -, the LZ4s stream's length and their quotient as measured when this file was made
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lz4s_format  # noqa: E402
import lz4s_sim  # noqa: E402
import refcalls  # noqa: E402

SEED = 11
CASES = [(k, 70001, SEED, 65536, mm) for k in ("text", "records", "silesia", "lzmix", "runs", "mod200", "rand", "allA") for mm in (3, 4)] + [
    ("text", 3073, SEED, 1024, 3), ("text", 3073, SEED, 1024, 4),
    ("silesia", 300000, SEED, 4096, 3), ("lzmix", 200000, SEED, 65536, 4),
    ("window", 131072, 5, 131072, 3), ("far65535", 131072, 6, 131072, 4), ("far65536", 131072, 6, 131072, 3),
    ("rand", 131072, SEED, 131072, 3), ("allA", 131072, SEED, 131072, 4),
    ("silesia", 524288 + 777, SEED, 524288, 3), ("records", 262144, SEED, 262144, 4),
]
RATIO = [(k, 262144, 7) for k in ("text", "records", "silesia", "lzmix")]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def main():
    assert refcalls.lz4_pinned(), "liblz4 1.9.3 is needed for the ratio records"
    out = {"cases": [], "ratio": []}
    for kind, n, seed, hw, mm in CASES:
        src = lz4s_sim.make_input(kind, n, seed)
        got, _ = lz4s_sim.compress(src, hw, mm)
        assert lz4s_format.decode(got, mm, hw) == src, (kind, n, hw, mm)
        out["cases"].append({"kind": kind, "n": n, "seed": seed, "hw_buff_sz": hw, "mini_match": mm, "in_sha": sha(src),
                             "out_len": len(got), "out_sha": sha(got)})
    for kind, n, seed in RATIO:
        src = lz4s_sim.make_input(kind, n, seed)
        bodies = sum(len(refcalls.lz4_compress_block(src[i:i + 65536], 65536 + 300)) for i in range(0, n, 65536))
        got, _ = lz4s_sim.compress(src, 65536, 3)
        out["ratio"].append({"kind": kind, "n": n, "seed": seed, "in_sha": sha(src), "lz4_bodies": bodies, "lz4s_len": len(got),
                             "ratio": round(len(got) / bodies, 4)})
    os.makedirs(os.path.join(HERE, "lz4s"), exist_ok=True)
    with open(os.path.join(HERE, "lz4s", "index.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for r in out["ratio"]:
        print(r["kind"], r["ratio"])


if __name__ == "__main__":
    main()
