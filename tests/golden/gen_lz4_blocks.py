#!/usr/bin/env python3
"""Creates tests/golden/lz4_blocks/: LZ4 frames of INDEPENDENT blocks and what liblz4 1.9.3's LZ4F_decompress answers to
hand-built ones - the ground truth of tests/test_sim_lz4_blocks.py and tests/test_gpu_lz4_blocks.py.  Run where liblz4
1.9.3 is installed; the output is committed.

index.json:
  files     whole frames LZ4F_compressFrame wrote with blockMode = independent (kept as files): input kind / n / seed, the
            preferences, SHA-256 of input and frame, the number of blocks
  verdicts  frames built by tests/lz4_frame_writer.py (verdict_frames() below builds them again in the tests): name, length
            and SHA-256 of the frame, and what LZ4F_decompress said - "OK" with length and SHA-256 of the output, or the
            library's error name.  cap_short = 1: the frame itself is fine, the test offers one byte less than it decodes to
"""
import ctypes
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import datagen  # noqa: E402
import lz4_frame_writer as W  # noqa: E402

MAXFILE = 150198

# (kind, n, seed, block id, block checksums, content checksum, content size)
FILES = (("text", 300000, 12, 4, 1, 1, 1), ("text", 300000, 12, 5, 1, 1, 1), ("allA", 9 << 20, 18, 7, 0, 1, 1),
         ("mod200", (2 << 20) + 4321, 19, 6, 1, 1, 1), ("rand", 70000, 15, 4, 1, 1, 1), ("text", 131073, 11, 4, 0, 1, 0),
         ("text", 131073, 11, 4, 1, 0, 1))


def sha(b):
    return hashlib.sha256(b).hexdigest()


def _text(n, seed):
    return datagen.gen_bytes("text", n, seed)


def verdict_frames():
    """[(name, frame bytes, cap_short)] - deterministic: datagen and the writer only.  Every frame is longer than 65571
    bytes, so that the device layer takes it for a candidate of the block route"""
    out = []
    a, b = _text(3000, 1), _text(1500, 2)
    big = datagen.gen_bytes("rand", 66000, 3)
    three = [(W.literals_block(a), False), (W.sequences_block([(b[:700], 300, 40)], b[700:]), False), (big, True)]
    content3 = a + b[:700] + bytes(b[400 + i % 300] for i in range(40)) + b[700:] + big
    for cc in (True, False):
        tag = "cc" if cc else "nocc"
        out.append(("three_blocks_" + tag, W.frame(three, content3, block_id=5, block_checksum=True, content_checksum=cc), 0))
        for k in range(3):
            blocks = [W.block(body, st, True, checksum_xor=(1 << (5 + 9 * k)) if j == k else 0) for j, (body, st) in enumerate(three)]
            out.append(("three_blocks_%s_badsum%d" % (tag, k), W.frame(blocks, content3, block_id=5, block_checksum=True, content_checksum=cc), 0))
    # a match of the second block that reaches into the first: refused in an independent frame, fine in a linked one
    first = _text(66000, 4)
    reach = [(W.literals_block(first), False), (W.sequences_block([(b"abc", 100, 8)], b"12345"), False)]
    whole = bytearray(first + b"abc")
    for _ in range(8):
        whole.append(whole[-100])
    whole += b"12345"
    out.append(("cross_block_independent", W.frame(reach, bytes(whole), block_id=5, independent=True, content_checksum=True), 0))
    out.append(("cross_block_linked", W.frame(reach, bytes(whole), block_id=5, independent=False, content_checksum=True), 0))
    # a dictID field, and nothing that reaches outside the frame
    two = [(W.literals_block(first), False), (W.sequences_block([(b[:500], 200, 30)], b[500:]), False)]
    content2 = first + b[:500] + bytes(b[300 + i % 200] for i in range(30)) + b[500:]
    out.append(("dict_id", W.frame(two, content2, block_id=5, content_checksum=True, content_size=len(content2), dict_id=0x12345678), 0))
    # a block of the BD maximum plus one byte behind a good one
    st = datagen.gen_bytes("rand", 65537 + 1000, 5)
    out.append(("block_above_bd_max", W.frame([(st[:1000], True), (st[1000:], True)], st, block_id=4, content_checksum=True), 0))
    # no end mark: the content checksum stands where a block word should
    st2 = datagen.gen_bytes("rand", 70000, 6)
    out.append(("end_mark_missing", W.frame([(st2[:40000], True), (st2[40000:], True)], st2, end_mark=False, block_id=4, content_checksum=True), 0))
    # more blocks than the frame's share of the block table
    tiny = _text(40000, 7)
    out.append(("8000_stored_blocks", W.frame([(tiny[5 * i:5 * i + 5], True) for i in range(8000)], tiny, block_id=4, block_checksum=True, content_checksum=True), 0))
    # a good frame for which the test has one byte too few
    out.append(("one_byte_short", W.frame(two, content2, block_id=5, block_checksum=True, content_checksum=True), 1))
    for name, fr, _ in out:
        assert len(fr) > 65571, (name, len(fr))
    return out


# ---------------------------------------------------------------- liblz4 (generator only)
def _lib():
    import refcalls
    assert refcalls.lz4_pinned(), "needs liblz4 1.9.3"
    lib = refcalls.lz4lib()
    lib.LZ4F_createDecompressionContext.restype = ctypes.c_size_t
    lib.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lib.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    lib.LZ4F_decompress.restype = ctypes.c_size_t
    lib.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_char_p,
                                    ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    lib.LZ4F_getErrorName.restype = ctypes.c_char_p
    lib.LZ4F_getErrorName.argtypes = [ctypes.c_size_t]
    return lib


def lz4f_decompress(frame, cap):
    """("OK", output) | (error name, None) | ("incomplete", None): one LZ4F_decompress call over the whole frame, as the
    reference makes it (src/qatzip_sw.c:496)"""
    lib = _lib()
    ctx = ctypes.c_void_p()
    assert not lib.LZ4F_isError(lib.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    dst = ctypes.create_string_buffer(max(cap, 1))
    dn, sn = ctypes.c_size_t(cap), ctypes.c_size_t(len(frame))
    r = lib.LZ4F_decompress(ctx, dst, ctypes.byref(dn), frame, ctypes.byref(sn), None)
    lib.LZ4F_freeDecompressionContext(ctx)
    if lib.LZ4F_isError(r):
        return lib.LZ4F_getErrorName(r).decode(), None
    if r != 0 or sn.value != len(frame):
        return "incomplete", None
    return "OK", dst.raw[:dn.value]


def compress_independent(src, block_id, bsum, csum, csize):
    import refcalls
    lib = _lib()
    prefs = refcalls._Prefs()
    prefs.frameInfo.blockMode = 1                                   # LZ4F_blockIndependent
    prefs.frameInfo.blockSizeID = block_id
    prefs.frameInfo.blockChecksumFlag = bsum
    prefs.frameInfo.contentChecksumFlag = csum
    prefs.frameInfo.contentSize = len(src) if csize else 0
    prefs.autoFlush = 1
    cap = lib.LZ4F_compressFrameBound(len(src), ctypes.byref(prefs))
    dst = ctypes.create_string_buffer(cap)
    r = lib.LZ4F_compressFrame(dst, cap, src, len(src), ctypes.byref(prefs))
    assert not lib.LZ4F_isError(r)
    return dst.raw[:r]


def main():
    d = os.path.join(HERE, "lz4_blocks")
    os.makedirs(d, exist_ok=True)
    idx = {"lz4": "1.9.3", "files": [], "verdicts": []}
    total = 0
    for kind, n, seed, bid, bsum, csum, csize in FILES:
        src = datagen.gen_bytes(kind, n, seed)
        fr = compress_independent(src, bid, bsum, csum, csize)
        assert fr[4] & 0x20 and (fr[5] >> 4) == bid, (kind, n, bid, hex(fr[4]), hex(fr[5]))
        v, back = lz4f_decompress(fr, n)
        assert v == "OK" and back == src
        name = "%s_%d_%d_b%d%s%s%s.lz4" % (kind, n, seed, bid, "_bc" if bsum else "", "_cc" if csum else "", "_cs" if csize else "")
        assert len(fr) <= MAXFILE, (name, len(fr))
        with open(os.path.join(d, name), "wb") as f:
            f.write(fr)
        total += len(fr)
        idx["files"].append({"kind": kind, "n": n, "seed": seed, "block_id": bid, "block_checksum": bsum, "content_checksum": csum,
                             "content_size": csize, "file": name, "in_sha": sha(src), "out_len": len(fr), "out_sha": sha(fr),
                             "blocks": len(W.blocks_of(fr)[0])})
        print("%-44s %8d B, %d blocks" % (name, len(fr), idx["files"][-1]["blocks"]))
    for name, fr, short in verdict_frames():
        v, back = lz4f_decompress(fr, 1 << 20)
        assert v != "incomplete", name                              # plainly an error or a success, nothing between
        rec = {"name": name, "len": len(fr), "sha": sha(fr), "liblz4": v, "cap_short": short}
        if v == "OK":
            rec["out_len"] = len(back); rec["out_sha"] = sha(back)
        idx["verdicts"].append(rec)
        print("%-32s %8d B  %s" % (name, len(fr), v))
    with open(os.path.join(d, "index.json"), "w") as f:
        json.dump(idx, f, indent=0)
    print("files: %d bytes" % total)


if __name__ == "__main__":
    main()
