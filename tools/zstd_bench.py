#!/usr/bin/env python3
"""Developer tool: zstd frames (Kz, qzd_zstd_compress_frames) on device-resident data, next to an LZ4s session's blocks
(K4s, qzd_lz4s_compress_blocks) on the same buffer in the same process, and the entropy stage alone
(qzd_zstd_encode_frames) next to the parse.

The data is bench.py's: 128 MiB of datagen's `silesia`, tiled with a period that is no multiple of a chunk.  Per
configuration one warm-up call, then --calls timed ones; GB/s is input bytes over the call's kernels, first to last, by HIP
events (qzd_last_timing), the best call; ratio is output bytes over input bytes.  The first frames of every zstd stream are
read back by the strict reader (tests/zstd_format.py).
The entropy stage alone: the records of the first --enc-mib MiB (from the LZ4s stream, by decLz4Block's rule, on the host),
repeated to the size of the buffer - the stage has no state across chunks, so equal chunks cost what different ones do - and
handed to qzd_zstd_encode_frames; its frames must be the ones qzd_zstd_compress_frames wrote for those chunks.
--seq-flags N (or a list, 0,1,2,3): every zstd line once per N through the _ex calls with those seq_flags
(include/qzamd_zstd_seq.h: 1 FSE_Compressed tables, 2 repeat offsets) instead of once through the calls without.
usage: zstd_bench.py [--mib 1024] [--calls 3] [--enc-mib 16] [--seq-flags N[,N...]]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen  # noqa: E402
import lz4s_format  # noqa: E402
import zstd_format  # noqa: E402
import zstd_full_format  # noqa: E402
import zstd_sim  # noqa: E402
import qatzip_amd  # noqa: E402
from qatzip_amd._lib import lz4s_bound  # noqa: E402

TILE_SKEW = 4099                    # as bench.py

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--enc-mib", type=int, default=16)
ap.add_argument("--seq-flags", default=None, help="seq_flags for the zstd calls, e.g. 3 or 0,1,2,3")
args = ap.parse_args()
FLAGS = [None] if args.seq_flags is None else [int(v) for v in args.seq_flags.split(",")]
n = args.mib << 20
base = datagen.gen("silesia", min(128 << 20, n), 20250523)
ctx = qatzip_amd.Context(0)
d_src = ctx.alloc(n)
tile = len(base) - TILE_SKEW if n > len(base) else len(base)
for off in range(0, n, tile):
    d_src.upload(base[:min(tile, n - off)], off)
d_c = ctx.alloc(lz4s_bound(n, 1024) + 4096)
print("%d MiB resident, silesia tiled so that no two chunks are equal; GB/s by HIP events, best of %d calls" % (args.mib, args.calls))


def run(what, call, size=n):
    out = call()
    ms = []
    for _ in range(args.calls):
        assert call() == out
        ms.append(ctx.timing()[3])
    print("%-52s %8.2f GB/s   ratio %.4f   (ms: %s)" % (what, size / (min(ms) * 1e-3) / 1e9, out / size, " / ".join("%.1f" % m for m in ms)),
          flush=True)
    return out, min(ms)


def tag(fl):
    return "" if fl is None else ", seq_flags %d" % fl


for hw in (65536, 131072):
    for mm in (3, 4):
        z_ms = []
        for fl in FLAGS:
            _, ms = run("Kz  zstd  %3d KB chunks, mini_match %d%s" % (hw >> 10, mm, tag(fl)),
                        lambda: ctx.zstd_compress_frames(d_src, n, d_c, hw, mm, 1, seq_flags=fl)[0])
            z_ms.append(ms)
            head = d_c.download(1 << 20).tobytes()
            src_head = d_src.download(4 * hw).tobytes()
            pos = 0
            for k in range(4):
                f, pos = zstd_full_format.decode_frame(head, pos) if fl else zstd_format.decode_frame(head, pos)
                assert f["data"] == src_head[k * hw:(k + 1) * hw]
        _, l_ms = run("K4s LZ4s  %3d KB chunks, mini_match %d" % (hw >> 10, mm), lambda: ctx.lz4s_compress_blocks(d_src, n, d_c, hw, mm, 1)[0])
        print("    (the first 4 frames decode to their input; zstd call / LZ4s call = %s)" % " / ".join("%.2f" % (z / l_ms) for z in z_ms), flush=True)

# the entropy stage alone, 64 KB chunks, mini_match 3
hw, mm = 65536, 3
m = min(args.enc_mib << 20, n)
_, lens = ctx.lz4s_compress_blocks(d_src, m, d_c, hw, mm, 1)
stream = d_c.download(int(lens.sum())).tobytes()
seqs, lits, desc = [], [], []
for b in lz4s_format.split(stream):
    s, l = zstd_sim.lz4s_records(b[4:], mm)
    seqs.append(np.array(s, dtype=np.uint32).reshape(-1, 3)); lits.append(l); desc.append((hw, len(s), len(l)))
reps = max(1, n // m)
seqs = np.tile(np.concatenate(seqs), (reps, 1)); lits = np.tile(np.frombuffer(b"".join(lits), np.uint8), reps)
desc = np.tile(np.array(desc, dtype=np.uint32), (reps, 1))
d_s = ctx.alloc(seqs.nbytes + 16); d_s.upload(seqs.tobytes())
d_l = ctx.alloc(lits.nbytes + 16); d_l.upload(lits.tobytes())
print("the entropy stage alone: %d frames of 64 KB, %.1f million records, %.1f MiB of literals" % (len(desc), len(seqs) / 1e6, lits.nbytes / 2**20))


for fl in FLAGS:
    zn, zlens = ctx.zstd_compress_frames(d_src, m, d_c, hw, mm, 1, seq_flags=fl)
    want = d_c.download(zn).tobytes()

    def enc():
        rc, out, _ = ctx.zstd_encode_frames(d_l, d_s, desc.reshape(-1), d_c, seq_flags=fl)
        assert rc == 0
        return out

    run("Kz  entropy stage alone (qzd_zstd_encode_frames)%s" % tag(fl), enc, size=reps * m)
    assert d_c.download(zn).tobytes() == want
    print("    (its first %d frames are the ones qzd_zstd_compress_frames wrote)" % len(zlens))
ctx.close()
