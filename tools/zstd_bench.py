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
--parse-depth D (or a list, 4,16,64): behind every zstd line one line per D through qzd_zstd_compress_frames_parse
(include/qzamd_zstd_parse.h: the hash-chain lazy parse with D search attempts per position), each followed by the default
parse again, so that the two alternate in one process; --mm and --chunks narrow the configurations, --no-enc leaves the
entropy stage alone out.
--libzstd: where libzstd loads, its ZSTD_compress on --threads threads (default 16) of this box, every chunk alone, on the
128 MiB the buffer is tiled from: ratio and rate per level 1 .. 19 and chunk size, then per Kzp line the lowest level whose
output is no larger than that line's, with its rate.
usage: zstd_bench.py [--mib 1024] [--calls 3] [--enc-mib 16] [--seq-flags N[,N...]] [--parse-depth D[,D...]] [--mm 3,4]
                     [--chunks 65536,131072] [--no-enc] [--libzstd] [--threads 16]"""
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
ap.add_argument("--parse-depth", default=None, help="parse depths for qzd_zstd_compress_frames_parse, e.g. 16 or 4,16,64")
ap.add_argument("--mm", default="3,4", help="the mini_match values to run")
ap.add_argument("--chunks", default="65536,131072", help="the chunk sizes to run")
ap.add_argument("--no-enc", action="store_true", help="skip the entropy stage alone")
ap.add_argument("--libzstd", action="store_true", help="libzstd's ZSTD_compress on --threads threads beside the Kzp lines")
ap.add_argument("--threads", type=int, default=16)
args = ap.parse_args()
DEPTHS = [] if args.parse_depth is None else [int(v) for v in args.parse_depth.split(",")]
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


KZP = []                            # (chunk size, line, ratio, GB/s) of every Kzp line


def libzstd_leg():
    """ZSTD_compress per chunk on args.threads threads (ctypes drops the GIL in the call): per chunk size the ratio and rate
    of every level on `base`, then the lowest level that is no larger than each Kzp line"""
    import ctypes as C
    import time
    from concurrent.futures import ThreadPoolExecutor
    import zstd_ref
    L = zstd_ref.lib()
    if not L:
        print("libzstd does not load here: no libzstd lines")
        return
    data = bytes(base)
    buf = C.create_string_buffer(data, len(data))
    addr, nt = C.addressof(buf), args.threads

    def work(a):
        lo, hi, hw, level = a
        cap = L.ZSTD_compressBound(hw)
        dst = C.create_string_buffer(cap)
        return sum(L.ZSTD_compress(dst, cap, C.c_char_p(addr + off), min(hw, hi - off), level) for off in range(lo, hi, hw))

    for hw in sorted(set(k[0] for k in KZP)) or [int(v) for v in args.chunks.split(",")]:
        per = (len(data) // hw + nt - 1) // nt * hw
        levels = {}
        for level in range(1, 20):
            t = time.time()
            with ThreadPoolExecutor(nt) as ex:
                tot = sum(ex.map(work, [(i, min(i + per, len(data)), hw, level) for i in range(0, len(data), per)]))
            dt = time.time() - t
            levels[level] = (tot / len(data), len(data) / dt / 1e9)
            print("libzstd %d  %3d KB chunks, level %2d, %d threads      %8.2f GB/s   ratio %.4f" % (zstd_ref.version(), hw >> 10, level, nt, levels[level][1], levels[level][0]), flush=True)
        for _, what, ratio, rate in (k for k in KZP if k[0] == hw):
            ok = [lv for lv in sorted(levels) if levels[lv][0] <= ratio]
            if ok:
                r, g = levels[ok[0]]
                print("    %s: %.2f GB/s at %.4f; libzstd's lowest level that is no larger: %d (%.4f) at %.2f GB/s on %d threads - %s" % (
                    what, rate, ratio, ok[0], r, g, nt, "this writer is SLOWER" if rate < g else "this writer is %.1f times faster" % (rate / g)), flush=True)
            else:
                print("    %s: %.2f GB/s at %.4f; no libzstd level up to 19 is as small" % (what, rate, ratio), flush=True)


def check_head(hw, full):
    head = d_c.download(1 << 20).tobytes()
    src_head = d_src.download(4 * hw).tobytes()
    pos = 0
    for k in range(4):
        f, pos = zstd_full_format.decode_frame(head, pos) if full else zstd_format.decode_frame(head, pos)
        assert f["data"] == src_head[k * hw:(k + 1) * hw]


for hw in [int(v) for v in args.chunks.split(",")]:
    for mm in [int(v) for v in args.mm.split(",")]:
        z_ms = []
        for fl in FLAGS:
            default = lambda: ctx.zstd_compress_frames(d_src, n, d_c, hw, mm, 1, seq_flags=fl)[0]
            _, ms = run("Kz  zstd  %3d KB chunks, mini_match %d%s" % (hw >> 10, mm, tag(fl)), default)
            z_ms.append(ms)
            check_head(hw, fl)
            for depth in DEPTHS:
                what = "Kzp zstd  %3d KB chunks, mini_match %d%s, depth %d" % (hw >> 10, mm, tag(fl), depth)
                out, ms = run(what, lambda: ctx.zstd_compress_frames(d_src, n, d_c, hw, mm, 1, seq_flags=fl, parse_depth=depth)[0])
                KZP.append((hw, what, out / n, n / (ms * 1e-3) / 1e9))
                check_head(hw, True)
                run("Kz  zstd  %3d KB chunks, mini_match %d%s (again)" % (hw >> 10, mm, tag(fl)), default)
        _, l_ms = run("K4s LZ4s  %3d KB chunks, mini_match %d" % (hw >> 10, mm), lambda: ctx.lz4s_compress_blocks(d_src, n, d_c, hw, mm, 1)[0])
        print("    (the first 4 frames decode to their input; zstd call / LZ4s call = %s)" % " / ".join("%.2f" % (z / l_ms) for z in z_ms), flush=True)

if args.libzstd:
    libzstd_leg()
if args.no_enc:
    ctx.close()
    sys.exit(0)
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
