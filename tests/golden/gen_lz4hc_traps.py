#!/usr/bin/env python3
"""Writes tests/golden/lz4hc_traps/index.json: per trap of tests/lz4hc_traps.py and per level of its `levels` the input's
SHA-256 and what liblz4 1.9.3's LZ4F_compressFrame (tests/refcalls.py: the reference's software path call) makes of it -
frame length and SHA-256, whether the trap's check held on it (`live`), and the decision labels of the serial model's trace.
It asserts that the model wrote liblz4's bytes on every trap at every level, and prints the label census: per label the
number of live traps that fire it.  Inputs are rebuilt from lz4hc_traps.py, never stored.  Run where liblz4.so.1 is 1.9.3.

  hw   the hardware-path records, after the `hw` scheme of gen_lz4hc.py: what follows the 15-byte header.  For a frame of one
       chunk that is the pinned frame from byte 15 on (block traps at their size class, linked traps at hw_buff_sz 262144);
       for the linked traps at hw_buff_sz 65536 it is recorded per 64 KB chunk.

  --search [count]   the seeded search over sm_input(): prints SM_SEEDS, per label the smallest input that fires it at every
                     level, and says which labels it never saw (every input it visits is also held against the library)
  --pairs            the colliding words
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lz4_traps as L1  # noqa: E402
import lz4hc_traps as T  # noqa: E402
import refcalls as R  # noqa: E402

OUT = os.path.join(HERE, "lz4hc_traps", "index.json")
LABEL_NO = {name: i for i, name in enumerate(T.LABELS)}


def sha(b):
    return hashlib.sha256(b).hexdigest()


def search(count):
    best = {}
    for n in T.SM_SIZES:
        for seed in range(count):
            src = T.sm_input(seed, n)
            per = []
            for lvl in (3, 8):
                frame, tr = T.model(src, lvl)
                assert frame == R.lz4f_compress_frame(src, lvl), ("model differs from liblz4", n, seed, lvl)
                per.append(set(tr.labels()))
            new = [lab for lab in per[0] & per[1] if lab not in best]
            if new:
                for lvl in (4, 5, 6, 7):
                    per.append(set(T.model(src, lvl)[1].labels()))
                for lab in set.intersection(*per):
                    best.setdefault(lab, (n, seed))
    print("SM_SEEDS = {")
    for lab in T.LABELS:
        if lab in best:
            print('    "%s": (%d, %d),' % (lab, best[lab][0], best[lab][1]))
    print("}")
    print("never seen in %d inputs per size:" % count, [lab for lab in T.LABELS if lab not in best])


def pairs():
    rs = np.random.RandomState(1)
    seen = {}
    while True:
        w = rs.randint(0, 256, 4, dtype=np.uint8).tobytes()
        h = T.hash_hc(T.u32(w, 0))
        hit = [o for o in seen.get(h, []) if o[2] != w[2] and o[3] != w[3]]
        if hit:
            print("COLLIDE", hit[0].hex(), w.hex())
            break
        seen.setdefault(h, []).append(w)
    hi = np.random.RandomState(2).randint(0, 256, 2, dtype=np.uint8).tobytes()
    seen = {}
    for lo in range(65536):
        w = bytes([lo & 255, lo >> 8]) + hi
        h = T.hash_hc(T.u32(w, 0))
        if h in seen and seen[h][0] != w[0] and seen[h][1] != w[1]:
            print("COLLIDE_LOW", seen[h].hex(), w.hex())
            break
        seen[h] = w
    rs = np.random.RandomState(3)
    while True:
        b = rs.randint(0, 256, 5, dtype=np.uint8).tobytes()
        if len(set(b)) == 5 and T.hash_hc(T.u32(b, 0)) == T.hash_hc(T.u32(b, 1)):
            print("COLLIDE_SHIFT", b.hex())
            break


def build():
    assert R.lz4_pinned(), "needs liblz4.so.1 1.9.3"
    traps, census = [], {lab: 0 for lab in T.LABELS}
    for t in T.all_traps():
        rec = {"name": t.name, "family": t.family, "n": len(t.data), "input_sha256": sha(t.data), "levels": {}}
        fires = set()
        for lvl in t.levels:
            frame = R.lz4f_compress_frame(t.data, lvl)
            mframe, tr = T.model(t.data, lvl)
            assert mframe == frame, ("model differs from liblz4", t.name, lvl)
            blocks = L1.parse_frame(frame)[2]
            live = bool(t.check(blocks, tr, lvl))
            if not live:
                print("NOT LIVE", t.name, lvl, t.aim)
            else:
                fires |= set(tr.labels())
            e = {"frame_len": len(frame), "frame_sha256": sha(frame), "live": live, "labels": sorted(LABEL_NO[x] for x in tr.labels())}
            if T.is_linked(t):
                e["hw65536"] = []
                for o in range(0, len(t.data), 65536):
                    fr = R.lz4f_compress_frame(t.data[o:o + 65536], lvl)
                    e["hw65536"].append({"len": len(fr) - 15, "sha": sha(fr[15:])})
            rec["levels"][str(lvl)] = e
        for lab in fires:
            census[lab] += 1
        traps.append(rec)
    print("label census (live traps that fire it):")
    for lab in T.LABELS:
        print("  %-18s %4d%s" % (lab, census[lab], "   (UNREACHABLE)" if lab in T.UNREACHABLE else ""))
    silent = [lab for lab in T.LABELS if not census[lab]]
    assert sorted(silent) == sorted(T.UNREACHABLE) and len(T.UNREACHABLE) <= 3, silent
    assert all(e["live"] for r in traps for e in r["levels"].values()), "a trap is not live"
    doc = {"liblz4": "1.9.3", "call": "LZ4F_compressFrame(contentChecksum, contentSize, autoFlush, levels 3-8)",
           "labels": list(T.LABELS), "census": census, "traps": traps}
    return json.dumps(doc, separators=(",", ":")).replace('{"name"', '\n{"name"') + "\n"


if __name__ == "__main__":
    if "--search" in sys.argv:
        search(int(sys.argv[sys.argv.index("--search") + 1]) if len(sys.argv) > sys.argv.index("--search") + 1 else 15000)
    elif "--pairs" in sys.argv:
        pairs()
    else:
        doc = build()
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(doc)
        print("wrote", OUT)
