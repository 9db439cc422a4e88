#!/usr/bin/env python3
"""Developer tool: one device-resident call of LZ4-HC (comp_lvl 3-8) as ONE linked frame, the data tools/lz4_bench.py builds.
Per level: one warm-up call, then three timed calls (host clock around the device-layer call, which ends in a device
synchronise) - all three printed.  With --cpu the same bytes go through liblz4 1.9.3 on 16 pinned workers, 64 KB-aligned
shares, one LZ4F_compressFrame each (when that library is installed; otherwise "CPU figure not measured").
usage: lz4hc_bench.py [--mib 1024] [--levels 3,6,8] [--cpu] [--calls 3]"""
import argparse
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen  # noqa: E402
import qatzip_amd  # noqa: E402
import refcalls  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--levels", default="3,6,8")
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--cpu", action="store_true")
args = ap.parse_args()
n = args.mib << 20
base = datagen.gen("silesia", min(128 << 20, n), 20250523)
ctx = qatzip_amd.Context(0)
d_src = ctx.alloc(n)
P = len(base) - 4099 if n > len(base) else len(base)
for off in range(0, n, P):
    d_src.upload(base[:min(P, n - off)], off)
d_c = ctx.alloc(n + 4 * (n >> 16) + 4096)
for lvl in (int(x) for x in args.levels.split(",")):
    cl = ctx.lz4_compress_linked(d_src, n, d_c, level=lvl)
    ts = []
    for _ in range(args.calls):
        t0 = time.perf_counter(); cl2 = ctx.lz4_compress_linked(d_src, n, d_c, level=lvl); ts.append(time.perf_counter() - t0)
        assert cl2 == cl
    print("lz4hc level %d, %d MiB, one linked frame: %s ms  (%s GB/s)  ratio %.4f  stream crc %08x"
          % (lvl, args.mib, " / ".join("%.1f" % (t * 1e3) for t in ts), " / ".join("%.2f" % (n / t / 1e9) for t in ts), cl / n,
             ctx.crc32(d_c, cl)), flush=True)
    if not args.cpu:
        continue
    if not refcalls.lz4_pinned():
        print("lz4hc level %d: CPU figure not measured (liblz4 1.9.3 is not installed here)" % lvl, flush=True)
        continue
    host = d_src.download(n).tobytes()
    W = 16
    share = ((n + W - 1) // W + 65535) & ~65535
    cpus = sorted(os.sched_getaffinity(0))
    outs = [0] * W

    def work(i):
        os.sched_setaffinity(0, {cpus[i % len(cpus)]})
        outs[i] = len(refcalls.lz4f_compress_frame(host[i * share:(i + 1) * share], lvl))
    th = [threading.Thread(target=work, args=(i,)) for i in range(W)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    print("lz4hc level %d, %d MiB, liblz4 1.9.3 on %d pinned workers (%d cpus allowed): %.1f ms (%.2f GB/s), %d bytes"
          % (lvl, args.mib, W, len(cpus), dt * 1e3, n / dt / 1e9, sum(outs)), flush=True)
