#!/usr/bin/env python3
"""Writes tests/golden/lz4_traps/index.json: per trap of tests/lz4_traps.py the input's SHA-256 and what liblz4 1.9.3's
LZ4F_compressFrame (tests/refcalls.py: the reference's software path call) makes of it - frame length and SHA-256, the
sequence list (a digest above 64 sequences), that the trap's check held on it, that LZ4_decompress_safe gave the input
back from every block, and that the serial model of lz4_traps.py read the same sequences.  Inputs are rebuilt from
lz4_traps.py, never stored.  Run where liblz4.so.1 is 1.9.3.   --search prints the seeds of the shrink-limit family."""
import ctypes
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lz4_traps as T  # noqa: E402
import refcalls as R  # noqa: E402

OUT = os.path.join(HERE, "lz4_traps", "index.json")


def sha(b):
    return hashlib.sha256(b).hexdigest()


def seq_record(blocks):
    flat = [[int(b.stored), b.raw, b.last, [list(s) for s in b.seqs]] for b in blocks]
    if sum(len(b.seqs) for b in blocks) > 64:
        return {"digest": sha(json.dumps(flat, separators=(",", ":")).encode())[:32], "count": sum(len(b.seqs) for b in blocks)}
    return flat


def blocks_decode(frame, src):
    """every compressed block through LZ4_decompress_safe (linked blocks with the 64 KB before them as prefix)"""
    lib = R.lz4lib()
    lib.LZ4_decompress_safe_usingDict.restype = ctypes.c_int
    lib.LZ4_decompress_safe_usingDict.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    p = 6 + (8 if frame[4] & 8 else 0) + 1
    pos = 0
    while True:
        bh = struct.unpack_from("<I", frame, p)[0]; p += 4
        if bh == 0:
            return pos == len(src)
        ln = bh & 0x7fffffff
        raw = min(65536, len(src) - pos)
        if bh >> 31:
            if frame[p:p + ln] != src[pos:pos + ln]:
                return False
            raw = ln
        else:
            dst = ctypes.create_string_buffer(raw)
            d = src[max(0, pos - 65536):pos]
            if d:
                r = lib.LZ4_decompress_safe_usingDict(frame[p:p + ln], dst, ln, raw, d, len(d))
            else:
                r = lib.LZ4_decompress_safe(frame[p:p + ln], dst, ln, raw)
            if r != raw or dst.raw != src[pos:pos + raw]:
                return False
        p += ln; pos += raw


def search():
    out = {}
    for n in (256, 1000, 4096, 65536):
        want = {-2: None, -1: None, 0: None, 1: None}
        seed = 0
        while any(v is None for v in want.values()):
            src = T.shrink_input(n, seed)
            d = len(R.lz4_compress_block(src, n + n // 255 + 64)) - n
            if d in want and want[d] is None:
                want[d] = seed
            seed += 1
        out[n] = want
    print("SHRINK_SEEDS =", out)


def build():
    assert R.lz4_pinned(), "needs liblz4.so.1 1.9.3"
    traps = []
    for t in T.all_traps():
        frame = R.lz4f_compress_frame(t.data, 1)
        _, _, blocks = T.parse_frame(frame)
        m = T.model(t.data)
        traps.append({"name": t.name, "family": t.family, "n": len(t.data), "mode": t.mode, "input_sha256": sha(t.data),
                      "frame_len": len(frame), "frame_sha256": sha(frame), "seqs": seq_record(blocks),
                      "live": bool(t.check(blocks)), "decodes": blocks_decode(frame, t.data),
                      "model_agrees": len(m) == len(blocks) and all(x[0] == b.stored and (b.stored or (x[1], x[2]) == (b.seqs, b.last))
                                                                        for x, b in zip(m, blocks)),
                      "fired": m[0][4] if t.name in T.G_FIRED else None})
    doc = {"liblz4": "1.9.3", "call": "LZ4F_compressFrame(contentChecksum, contentSize, autoFlush, level 1)", "traps": traps}
    return json.dumps(doc, separators=(",", ":")).replace('{"name"', '\n{"name"') + "\n"


if __name__ == "__main__":
    if "--search" in sys.argv:
        search()
    else:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(build())
        print("wrote", OUT)
