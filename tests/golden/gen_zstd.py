#!/usr/bin/env python3
"""Creates tests/golden/zstd/index.json: what the zstd kernel (qatzip_amd/csrc/qzk_zstd.h) writes on the CPU SIMT emulator for
a fixed list of inputs - the pin tests/test_sim_zstd.py reproduces on the emulator and tests/test_gpu_zstd.py on the GPU (the
two builds must give the same bytes).  Every pinned stream was decoded by the strict reader (tests/zstd_format.py) and by
libzstd's ZSTD_decompress when this file was made.  Run it again only when the parse or the entropy stage is changed on
purpose; the output is committed.

index.json:
  cases   (kind, n, seed, hw_buff_sz, mini_match): input SHA-256, stream length, stream SHA-256
  ratio   for the corpora of the LZ4s ratio gate (262144 bytes, 64 KB chunks, mini_match 3): this encoder's total, the LZ4s
          stream's, libzstd's ZSTD_compress level-1 total over the same chunks, and - the reference's exact path - libzstd's
          ZSTD_compressSequences total with explicit block delimiters on the same sequences (null where the library refuses
          the call); ratio = this encoder's total over the latter, cap = ratio + 0.02, which the test asserts
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lz4s_sim  # noqa: E402
import zstd_format  # noqa: E402
import zstd_ref  # noqa: E402
import zstd_sim  # noqa: E402

SEED = 11
CASES = [(k, 70001, SEED, 65536, mm) for k in ("text", "records", "silesia", "lzmix", "runs", "mod200", "rand", "allA") for mm in (3, 4)] + [
    ("text", 3073, SEED, 1024, 3), ("text", 3073, SEED, 1024, 4),
    ("silesia", 300000, SEED, 4096, 3), ("lzmix", 200000, SEED, 65536, 4),
    ("window", 131072, 5, 131072, 3), ("far65535", 131072, 6, 131072, 4), ("far65536", 131072, 6, 131072, 3),
    ("rand", 131072, SEED, 131072, 3), ("allA", 131072, SEED, 131072, 4), ("merged", 73000, 8, 131072, 3),
    ("silesia", 131072 + 777, SEED, 131072, 3), ("records", 262144, SEED, 16384, 4),
]
RATIO = [(k, 262144, 7) for k in ("text", "records", "silesia", "lzmix")]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def main():
    assert zstd_ref.available(), "libzstd is needed for the ratio records and the second decode"
    out = {"libzstd": zstd_ref.version(), "cases": [], "ratio": []}
    for kind, n, seed, hw, mm in CASES:
        src = zstd_sim.make_input(kind, n, seed)
        got, _ = zstd_sim.compress(src, hw, mm)
        assert zstd_format.decode(got, hw) == src, (kind, n, hw, mm)
        zstd_ref.check(got, src)
        out["cases"].append({"kind": kind, "n": n, "seed": seed, "hw_buff_sz": hw, "mini_match": mm, "in_sha": sha(src),
                             "out_len": len(got), "out_sha": sha(got)})
    for kind, n, seed in RATIO:
        src = zstd_sim.make_input(kind, n, seed)
        got, _ = zstd_sim.compress(src, 65536, 3)
        l4s, _ = lz4s_sim.compress(src, 65536, 3)
        seqs = zstd_sim.expected_sequences(src, 65536, 3)
        chunks = [src[i:i + 65536] for i in range(0, n, 65536)]
        level1 = sum(len(zstd_ref.compress(c, 1)) for c in chunks)
        zs = [zstd_ref.compress_sequences(c, s) for c, s in zip(chunks, seqs)]
        for c, z in zip(chunks, zs):
            if z is not None:
                assert zstd_ref.decompress(z, len(c)) == c
        zseq = None if any(z is None for z in zs) else sum(len(z) for z in zs)
        base = zseq if zseq is not None else level1
        ratio = round(len(got) / base, 4)
        out["ratio"].append({"kind": kind, "n": n, "seed": seed, "in_sha": sha(src), "zstd_len": len(got), "lz4s_len": len(l4s),
                             "libzstd_level1": level1, "libzstd_compress_sequences": zseq, "ratio": ratio,
                             "cap": round(ratio + 0.02, 4)})
    os.makedirs(os.path.join(HERE, "zstd"), exist_ok=True)
    with open(os.path.join(HERE, "zstd", "index.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for r in out["ratio"]:
        print(r)


if __name__ == "__main__":
    main()
