#!/usr/bin/env python3
"""Creates tests/golden/lz4hc/: what liblz4 1.9.3's LZ4F_compressFrame writes at compression levels 3-8 (LZ4-HC) with the
preferences of the reference's software path (tests/refcalls.py::lz4f_compress_frame) - the ground truth of
tests/test_sim_lz4hc.py and tests/test_gpu_lz4hc.py.  Run where liblz4 1.9.3 is installed; the output is committed.

index.json:
  cases   every datagen kind x N x level 3-8: input SHA-256, frame length, frame SHA-256, the frame's block-size words
  edge    inputs that barely shrink (random bytes with planted 5-8 byte repeats, found by a seed search with the library):
          per size the block nearest below the n - 1 limit (compressed) and the one nearest above it (stored in the frame);
          the input is rebuilt by barely(seed, n) below
  files   whole frames kept as files: the inputs of tests/golden/lz4_linked at levels 3 and 8
  hw      hardware-path framing: per hw_buff_sz chunk, length and SHA-256 of the library's frame for that chunk from byte 15
          on (block words, blocks, end mark, content checksum - what follows the 15-byte header)
  big     one 256 MiB call at level 6: total length and 64 blocks (length, SHA-256 of the body) at fixed indices
"""
import hashlib
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import datagen  # noqa: E402
import refcalls  # noqa: E402

NS = (0, 1, 12, 13, 4000, 65535, 65536, 65537, 65536 + 12, 131072, 131073, 200777, 300000, 1 << 20)
LEVELS = (3, 4, 5, 6, 7, 8)
SEED = 41
BIG = {"kind": "silesia", "n": 256 << 20, "seed": 77, "level": 6}
BIG_BLOCKS = [0, 1, 2, 3] + [64 * i + (i * 37) % 64 for i in range(1, 59)] + [4094, 4095]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def blocks_of(frame):
    """[(word, body offset, body length)] of a frame with content size (15-byte header)"""
    pos = 15 if frame[4] & 8 else 7
    out = []
    while True:
        w = struct.unpack_from("<I", frame, pos)[0]
        pos += 4
        if w == 0:
            return out
        ln = w & 0x7fffffff
        out.append((w, pos, ln))
        pos += ln


def barely(seed, n):
    """random bytes with sparse planted repeats"""
    rng = random.Random(seed)
    b = bytearray(rng.randbytes(n))
    for _ in range(rng.randrange(20, 81) * max(1, n // 30000)):
        ln = rng.randrange(5, 9)
        a = rng.randrange(0, n - 2 * ln)
        d = rng.randrange(a + ln, n - ln)
        b[d:d + ln] = b[a:a + ln]
    return bytes(b)


def hc_block_sizes(src, level):
    """sizes of the 64 KB blocks of src as LZ4_compress_HC_continue writes them when the destination has room to spare"""
    import ctypes
    lib = refcalls.lz4lib()
    lib.LZ4_createStreamHC.restype = ctypes.c_void_p
    lib.LZ4_resetStreamHC_fast.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.LZ4_compress_HC_continue.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.LZ4_freeStreamHC.argtypes = [ctypes.c_void_p]
    st = lib.LZ4_createStreamHC()
    lib.LZ4_resetStreamHC_fast(st, level)
    buf = ctypes.create_string_buffer(src, len(src))
    dst = ctypes.create_string_buffer(70000)
    out = []
    for o in range(0, len(src), 65536):
        out.append(lib.LZ4_compress_HC_continue(st, ctypes.addressof(buf) + o, dst, min(65536, len(src) - o), 70000))
    lib.LZ4_freeStreamHC(st)
    return out


def main():
    assert refcalls.lz4_pinned(), "needs liblz4 1.9.3"
    d = os.path.join(HERE, "lz4hc")
    os.makedirs(d, exist_ok=True)
    idx = {"lz4": "1.9.3", "cases": [], "edge": [], "files": [], "hw": [], "big": None}
    for kind in datagen.KINDS:
        for n in NS:
            src = datagen.gen_bytes(kind, n, SEED)
            for lvl in LEVELS:
                fr = refcalls.lz4f_compress_frame(src, lvl)
                idx["cases"].append({"kind": kind, "n": n, "seed": SEED, "level": lvl, "in_sha": sha(src), "out_len": len(fr),
                                     "out_sha": sha(fr), "words": [w for w, _, _ in blocks_of(fr)]})
    # block-store edges: one full 64 KB block, a short single block, and a short last block behind a full one.  The margin is
    # the last block's size with room to spare (LZ4_compress_HC_continue, same parse) minus the n - 1 the frame allows it.
    for n, level in ((65536, 6), (65536, 3), (30000, 6), (65536 + 30000, 6), (65536 + 30000, 8)):
        best = {}                                                   # "under" / "over" -> (margin, seed)
        for seed in range(1, 161):
            src = barely(seed, n)
            bn = n - (n - 1) // 65536 * 65536                       # the last block's bytes
            m = hc_block_sizes(src, level)[-1] - (bn - 1)
            which = "over" if m > 0 else "under"
            if which not in best or abs(m) < abs(best[which][0]):
                best[which] = (m, seed)
        for which, (m, seed) in sorted(best.items()):
            src = barely(seed, n)
            fr = refcalls.lz4f_compress_frame(src, level)
            words = [w for w, _, _ in blocks_of(fr)]
            assert bool(words[-1] & 0x80000000) == (which == "over"), (n, level, seed, m)
            idx["edge"].append({"n": n, "seed": seed, "level": level, "outcome": which, "margin": m, "in_sha": sha(src),
                                "out_len": len(fr), "out_sha": sha(fr), "words": words})
    with open(os.path.join(HERE, "lz4_linked", "index.json")) as f:
        linked = json.load(f)["frames"]
    for fr0 in linked:
        src = datagen.gen_bytes(fr0["kind"], fr0["n"], fr0["seed"])
        for lvl in (3, 8):
            fr = refcalls.lz4f_compress_frame(src, lvl)
            name = "%s_%d_%d_L%d.lz4" % (fr0["kind"], fr0["n"], fr0["seed"], lvl)
            assert len(fr) <= 150198, name
            with open(os.path.join(d, name), "wb") as f:
                f.write(fr)
            idx["files"].append({"kind": fr0["kind"], "n": fr0["n"], "seed": fr0["seed"], "level": lvl, "file": name,
                                 "in_sha": sha(src), "out_len": len(fr), "out_sha": sha(fr)})
    for kind, n, seed in (("text", 600000, 51), ("silesia", 1 << 20, 52), ("rand", 300000, 53), ("records", 262144 + 5, 54)):
        src = datagen.gen_bytes(kind, n, seed)
        for hw in (65536, 262144):
            for lvl in (3, 6, 8):
                chunks = []
                for o in range(0, n, hw):
                    fr = refcalls.lz4f_compress_frame(src[o:o + hw], lvl)
                    chunks.append({"len": len(fr) - 15, "sha": sha(fr[15:])})
                idx["hw"].append({"kind": kind, "n": n, "seed": seed, "level": lvl, "hw_buff_sz": hw, "in_sha": sha(src), "chunks": chunks})
    src = datagen.gen_bytes(BIG["kind"], BIG["n"], BIG["seed"])
    fr = refcalls.lz4f_compress_frame(src, BIG["level"])
    bl = blocks_of(fr)
    assert len(bl) == 4096
    idx["big"] = dict(BIG, in_sha=sha(src), out_len=len(fr),
                      blocks=[{"index": i, "word": bl[i][0], "sha": sha(fr[bl[i][1]:bl[i][1] + bl[i][2]])} for i in sorted(set(BIG_BLOCKS))])
    assert len(idx["big"]["blocks"]) == 64, len(idx["big"]["blocks"])
    with open(os.path.join(d, "index.json"), "w") as f:
        json.dump(idx, f, indent=0)
    print("%d cases, %d edge, %d files, %d hw, big %d -> %d" % (len(idx["cases"]), len(idx["edge"]), len(idx["files"]), len(idx["hw"]),
                                                                 BIG["n"], len(fr)))


if __name__ == "__main__":
    main()
