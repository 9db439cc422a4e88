"""The zstd kernels (qatzip_amd/csrc/qzk_zstd.h) on the CPU SIMT emulator, and what the zstd tests share: used by
tests/test_sim_zstd.py, tests/test_gpu_zstd.py and tests/golden/gen_zstd.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import lz4s_format
import lz4s_sim
import zstd_format

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)
SO = os.path.join(SIMDIR, "libqzsim_zstd.so")
INDEX = os.path.join(HERE, "golden", "zstd", "index.json")
ERR_PARAM, ERR_DATA = -10, -11

_S = None


def _deps():
    deps = [os.path.join(SIMDIR, f) for f in ("sim_zstd.cpp", "hipsim.h")]
    csrc = os.path.join(ROOT, "qatzip_amd", "csrc")
    return deps + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]


def build_so():
    """g++ build of tests/sim/sim_zstd.cpp, redone when a source is newer"""
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in _deps()):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-I", SIMDIR, "-Wno-unused-function",
                               "-o", SO, os.path.join(SIMDIR, "sim_zstd.cpp")])
    return SO


def _load():
    global _S
    if _S is None:
        S = C.CDLL(build_so())
        S.sim_zstd.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                               C.POINTER(C.c_uint64), C.c_void_p]
        S.sim_zstd_encode.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64), C.c_void_p]
        S.sim_zstd_bound.argtypes = [C.c_uint64, C.c_uint32]
        S.sim_zstd_bound.restype = C.c_uint64
        _S = S
    return _S


def compress(src, hw_buff_sz=65536, mini_match=3, waves=0):
    """-> (stream of frames, per-frame lengths).  The driver itself checks that no frame passes its bound and that nothing
    is written behind it (rc -3)."""
    S = _load()
    n = len(src)
    nb = (n + hw_buff_sz - 1) // hw_buff_sz
    cap = zstd_format.bound(n, hw_buff_sz)
    assert cap == S.sim_zstd_bound(n, hw_buff_sz)
    out = C.create_string_buffer(cap + 64)
    ol = C.c_uint64(0)
    lens = (C.c_uint32 * max(nb, 1))()
    rc = S.sim_zstd(src, n, hw_buff_sz, mini_match, waves, out, cap, C.byref(ol), lens)
    assert rc == 0, "sim_zstd rc=%d" % rc
    return out.raw[:ol.value], list(lens)[:nb]


def pack_frames(frames):
    """[(content size, [(ll, ml, off)], literal bytes)] -> (literals, records as uint32 x 3, descriptions as uint32 x 3)"""
    lits = b"".join(f[2] for f in frames)
    seqs = np.array([v for f in frames for s in f[1] for v in s], dtype=np.uint32)
    desc = np.array([v for f in frames for v in (f[0], len(f[1]), len(f[2]))], dtype=np.uint32)
    return lits, seqs, desc


def encode(frames, waves=0):
    """the entropy stage alone on hand-made records -> (rc, stream, per-frame lengths); rc ERR_PARAM / ERR_DATA where the
    device layer answers QZD_ERR_PARAM / QZD_ERR_DATA"""
    S = _load()
    lits, seqs, desc = pack_frames(frames)
    cap = sum(min(f[0], zstd_format.MAX_BLOCK) + 12 for f in frames)
    out = C.create_string_buffer(cap + 64)
    ol = C.c_uint64(0)
    lens = (C.c_uint32 * max(len(frames), 1))()
    seqs = np.concatenate([seqs, np.zeros(3, np.uint32)])
    rc = S.sim_zstd_encode(lits + b"\0", seqs.ctypes.data, desc.ctypes.data, len(frames), waves, out, cap, C.byref(ol), lens)
    return rc, out.raw[:ol.value], list(lens)[:len(frames)]


def lz4s_records(blk, mini_match):
    """decLz4Block's rule (the reference's utils/qzstd.c:118-179) on one LZ4s block's sequences (without the size word) ->
    ([(literal length, match length, offset)], the literal bytes): the literals of an M == 0 sequence join the next one, the
    block's trailing literals are in no record"""
    pos, pend, out, lits = 0, 0, [], []
    while pos < len(blk):
        token = blk[pos]
        pos += 1
        L = token >> 4
        if L == 15:
            L, pos = lz4s_format._ext(blk, pos, L)
        lits.append(blk[pos:pos + L])
        pos += L
        pend += L
        if pos == len(blk):
            break
        offset = blk[pos] | blk[pos + 1] << 8
        pos += 2
        M = token & 15
        if M == 15:
            M, pos = lz4s_format._ext(blk, pos, M)
        if M:
            out.append((pend, M + mini_match - 1, offset))
            pend = 0
    return out, b"".join(lits)


def lz4s_sequences(blk, mini_match):
    return lz4s_records(blk, mini_match)[0]


def expected_sequences(src, hw_buff_sz, mini_match):
    """per chunk, what decLz4Block's rule yields from the LZ4s session's stream for the same input"""
    stream, _ = lz4s_sim.compress(src, hw_buff_sz, mini_match)
    return [lz4s_sequences(b[4:], mini_match) for b in lz4s_format.split(stream)]


def merged_input(seed=8):
    """70000 random bytes followed by a repeat of 3000 of them (a source the table still holds): one sequence whose merged
    literal length is above 65535 - LL code 35"""
    r = lz4s_sim._rand(70000, seed)
    return r + r[66000:69000]


def make_input(kind, n, seed):
    """lz4s_sim's kinds, and "merged" (n = 73000)"""
    if kind == "merged":
        assert n == 73000
        return merged_input(seed)
    return lz4s_sim.make_input(kind, n, seed)


def index():
    with open(INDEX) as f:
        return json.load(f)


# ---------------------------------------------------------------- hand-made records for the entropy stage's edges
def rebuild(frame):
    """what a frame (content size, records, literals) stands for, in plain Python"""
    _, seqs, lits = frame
    out, lp = bytearray(), 0
    for ll, ml, off in seqs:
        out += lits[lp:lp + ll]
        lp += ll
        assert 1 <= off <= len(out)
        for _ in range(ml):
            out.append(out[-off])
    out += lits[lp:]
    return bytes(out)


def patterned(n, mod=251, mul=7):
    return bytes((i * mul) % mod for i in range(n))


def skewed(n, top=40, seed=3):
    """n bytes over the symbols 0 .. top with falling frequency (a Huffman code pays), `top` itself present"""
    g = np.random.Generator(np.random.PCG64([seed, n, top]))
    v = np.minimum(g.geometric(0.12, n) - 1, top).astype(np.uint8)
    v[n // 2] = top
    return v.tobytes()


def one_match(lits, ml=100, off=1, trailing=b""):
    """every literal in front of one match, then `trailing`"""
    return (len(lits) + ml + len(trailing), [(len(lits), ml, off)], lits + trailing)


def many(count, ml=3):
    """`count` records of one literal and a match of ml at offset 1"""
    lits = bytes(65 + (i * 5) % 23 for i in range(count))
    return (count * (1 + ml), [(1, ml, 1)] * count, lits)


def fibonacci_literals(symbols=20):
    """counts 1, 1, 2, 3, 5 ... over `symbols` symbols: an unlimited Huffman code is symbols - 1 bits deep"""
    a, b, out = 1, 1, bytearray()
    for s in range(symbols):
        out += bytes([s]) * a
        a, b = b, a + b
    g = np.random.Generator(np.random.PCG64([5, symbols]))
    v = np.frombuffer(bytes(out), np.uint8).copy()
    g.shuffle(v)
    return v.tobytes()


EDGES = {
    # sequence counts: the 1-, 2- and 3-byte forms
    "count0": (500, [], skewed(500)), "count1": one_match(skewed(50)), "count127": many(127), "count128": many(128),
    "count7eff": many(0x7eff), "count7f00": many(0x7f00),
    # Raw literals at the size formats' edges (a literals section of 0 bytes cannot be: the first match needs a byte)
    "raw31": one_match(patterned(31)), "raw32": one_match(patterned(32)), "raw4095": one_match(patterned(4095, 256, 1)),
    "raw4096": one_match(patterned(4096, 256, 1)),
    # Compressed literals: one stream / four, the 14- and 18-bit headers
    "huf1023": one_match(skewed(1023)), "huf1024": one_match(skewed(1024)), "huf16383": one_match(skewed(16383)),
    "huf16384": one_match(skewed(16384)),
    "rle": one_match(b"x" * 300), "two": one_match(bytes([7, 9, 9, 9] * 200)), "uniform256": one_match(patterned(8192, 256, 1)),
    "fibonacci": one_match(fibonacci_literals(20)),
    "top127": one_match(skewed(3000, 127)), "top128": one_match(skewed(3000, 128)), "top129": one_match(skewed(3000, 129)),
    "top255": one_match(skewed(3000, 255)),
    # (short frames: one literal value, so that the block is smaller than its content and stays Compressed)
    "ml3": one_match(b"q" * 40, 3), "ml4": one_match(b"q" * 40, 4), "ml34": one_match(b"q" * 40, 34), "ml35": one_match(b"q" * 40, 35),
    "ml65535": one_match(skewed(40), 65535, 5),
    "ll15": one_match(b"q" * 15), "ll16": one_match(b"q" * 16), "ll63": one_match(b"q" * 63), "ll64": one_match(b"q" * 64),
    "ll65535": one_match(skewed(65535), 100, 65535), "ll65536": one_match(skewed(65536)),
    "ll131069": one_match(skewed(131069), 3, 5),                    # the longest a 128 KB frame with a match holds
    "off1": one_match(skewed(40), 50, 1), "off5": one_match(skewed(40), 50, 5), "trailing": one_match(skewed(40), 50, 5, b"tail" * 10),
}
# what qzd_zstd_encode_frames refuses, and how
REFUSED = {
    "sum_short": ((10, [(4, 5, 1)], b"abcd"), ERR_DATA), "sum_long": ((8, [(4, 5, 1)], b"abcd"), ERR_DATA),
    "offset0": ((9, [(4, 5, 0)], b"abcd"), ERR_DATA), "offset_beyond": ((9, [(4, 5, 5)], b"abcd"), ERR_DATA),
    "offset_beyond_2nd": ((17, [(4, 5, 1), (0, 8, 10)], b"abcd"), ERR_DATA),
    "match2": ((10, [(4, 2, 1), (0, 4, 1)], b"abcd"), ERR_DATA), "no_literals": ((6, [(0, 6, 1)], b""), ERR_DATA),
    "literals_short": ((9, [(4, 5, 1)], b"abc"), ERR_DATA),
    "content_above_128k": ((131073, [(131070, 3, 5)], bytes(131070)), ERR_PARAM),
    "ll131071": ((131074, [(131071, 3, 5)], bytes(131071)), ERR_PARAM),    # a literal length of 131071 needs 131074 bytes of content
    "content0": ((0, [], b""), ERR_PARAM), "literals_above_content": ((6, [], b"abcdefg"), ERR_PARAM),
    "records_above_a_third": ((6, [(0, 3, 1)] * 3, b""), ERR_PARAM),
}
