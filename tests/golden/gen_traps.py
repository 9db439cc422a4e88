#!/usr/bin/env python3
"""Generate tests/golden/traps.json: libz 1.2.11's own bytes for every trap input of tests/deflate_traps.py.

Run where the system libz is 1.2.11 (tests/test_sim_deflate_traps.py regenerates the file and compares it byte for
byte there, and skips elsewhere).  Driven exactly like the existing goldens (tests/refcalls.py: one deflate() +
Z_FULL_FLUSH per hw_buff_sz chunk, Z_FINISH on the last when `last`).  The inputs themselves are not stored: the
generator rebuilds them from its fixed seeds, and every case records its input's SHA-256 so that a changed generator
is caught.  Digests are SHA-256 cut to 24 hex digits (96 bits; 16 for the inputs), which keeps the file small.

runs: [name, fmt, level, hw, last, out_len, out_sha, out_hex or ""] - every case at each of its levels with its own hw
and last = 1; a subset with last = 0; a subset at small hw (several chunks); a handful as GZIP_EXT members.
"""
import hashlib
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import deflate_traps as T  # noqa: E402
import refcalls as R  # noqa: E402

OUT = os.path.join(HERE, "traps.json")
HEX_MAX = 24          # outputs up to this many bytes are stored whole


def sha(b, n=24):
    return hashlib.sha256(b).hexdigest()[:n]


def plan(cases):
    """(case, fmt, level, hw, last) of every golden run"""
    runs = []
    for i, c in enumerate(cases):
        for lv in c.levels:
            runs.append((c, "RAW", lv, c.hw, 1))
        if i % 7 == 3:
            runs.append((c, "RAW", c.levels[0], c.hw, 0))
        if i % 23 == 5 and len(c.data) > 1024:
            runs.append((c, "RAW", c.levels[0], 1024 if len(c.data) < 20000 else 16384, 1))
        if i % 97 == 11:
            runs.append((c, "GZIP_EXT", c.levels[0], c.hw, 1))
    return runs


def compress(fmt, data, level, hw, last):
    if fmt == "RAW":
        return b"".join(R.raw_chunks(data, hw, level, last))
    return R.sw_compress(R.FMT_GZIP_EXT, data, hw, level, last)


def build():
    cases = T.all_cases()
    doc = {"zlib": zlib.ZLIB_RUNTIME_VERSION, "generator": "tests/golden/gen_traps.py",
           "cases": {c.name: [len(c.data), sha(c.data, 16)] for c in cases}, "runs": []}
    for c, fmt, lv, hw, last in plan(cases):
        out = compress(fmt, c.data, lv, hw, last)
        doc["runs"].append([c.name, fmt, lv, hw, last, len(out), sha(out), out.hex() if len(out) <= HEX_MAX else ""])
    return json.dumps(doc, separators=(",", ":"), sort_keys=True) + "\n"


def main():
    assert R.zlib_pinned() and R.libz_pinned(), "need libz 1.2.11"
    text = build()
    with open(OUT, "w") as f:
        f.write(text)
    print(len(json.loads(text)["runs"]), "runs", len(text), "bytes")


if __name__ == "__main__":
    main()
