#!/usr/bin/env python3
"""Creates tests/golden/lz4_sequences/index.json: what liblz4 1.9.3's LZ4F_decompress answers to every frame of the
sequence matrix (tests/lz4_blocks_cases.py) - the ground truth of tests/test_sim_lz4_sequences.py and
tests/test_gpu_lz4_sequences.py.  Run where liblz4 1.9.3 is installed (python3 tests/golden/gen_lz4_sequences.py); the
index is committed, the frames are not: the tests build them again and hold them against the SHAs here.

index.json, "cases": one entry per case - name, class (set by the builder, never by the result), and per wrapping ("wave",
"blocks"; linked frames have the first only): length and SHA-256 of the frame, the capacity offered, and what ONE
LZ4F_decompress call over the whole frame at that capacity said - "OK" with length and SHA-256 of the output, the library's
error name, or "incomplete" (no error, and the frame not through: the capacity is too small).

Wherever liblz4 says OK and the builder has a model, the two must be the same bytes: that holds the builder's byte-by-byte
LZ77 copy against the reference, here, once."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import lz4_blocks_cases as K  # noqa: E402
from gen_lz4_blocks import lz4f_decompress  # noqa: E402


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def judge(case, wrapping):
    """(frame, index record) of one wrapping"""
    fr, cap = case.frame(wrapping), case.cap(wrapping)
    v, back = lz4f_decompress(fr, cap)
    rec = {"len": len(fr), "sha": sha(fr), "cap": cap, "liblz4": v}
    if v == "OK":
        rec["out_len"] = len(back); rec["out_sha"] = sha(back)
        want = case.content(wrapping)
        if case.cls != K.OFFSET0:                                   # (offset 0: liblz4 copies from memory that is not the frame's)
            assert want is not None, (case.name, wrapping, "liblz4 decodes what the model refuses")
            assert back == want, (case.name, wrapping, "the model and liblz4 disagree")
    return fr, rec


def main():
    d = os.path.join(HERE, "lz4_sequences")
    os.makedirs(d, exist_ok=True)
    idx = {"lz4": "1.9.3", "cases": []}
    said = {}
    for c in K.cases():
        rec = {"name": c.name, "class": c.cls}
        for w in c.wrappings():
            _, rec[w] = judge(c, w)
            said.setdefault((c.cls, rec[w]["liblz4"]), []).append(c.name)
        if c.cls == K.STRICT and c.model is not None and c.cap_delta >= 0:
            assert all(rec[w]["liblz4"] == "OK" for w in c.wrappings()), (c.name, rec)     # a valid block that obeys the end rules
        idx["cases"].append(rec)
    with open(os.path.join(d, "index.json"), "w") as f:
        json.dump(idx, f, indent=0)
    for (cls, v), names in sorted(said.items()):
        print("%-16s %-32s %4d  %s" % (cls, v, len(names), " ".join(sorted(set(names))[:4])))
    print("%d cases" % len(idx["cases"]))


if __name__ == "__main__":
    main()
