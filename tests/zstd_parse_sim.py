"""The hash-chain lazy parse of zstd sessions (include/qzamd_zstd_parse.h, qatzip_amd/csrc/qzk_zstd_parse.h) on the CPU SIMT
emulator, and what the tests of the option share: used by tests/test_sim_zstd_parse.py, tests/test_gpu_zstd_parse.py and
tests/golden/gen_zstd_parse.py."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np

import zstd_format
import zstd_sim as S
import zstd_seq_sim as Q

SO = os.path.join(S.SIMDIR, "libqzsim_zstd_parse.so")
SRC = os.path.join(S.SIMDIR, "sim_zstd_parse.cpp")
INDEX = os.path.join(S.HERE, "golden", "zstd_parse", "index.json")
MAX_DEPTH = 256
DEPTHS = (1, 4, 16, 64, 256)

_S = None


def build_so():
    """g++ build of tests/sim/sim_zstd_parse.cpp, redone when a source is newer"""
    deps = [SRC] + [d for d in S._deps() if not d.endswith("sim_zstd.cpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-I", S.SIMDIR, "-Wno-unused-function",
                               "-o", SO, SRC])
    return SO


def load(path):
    """the emulator library at `path` with its argument types (a build of SRC with other -D values: a mutant)"""
    L = C.CDLL(path)
    L.sim_zstd_parse.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                 C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sim_zstd_parse_round.argtypes = [C.c_uint32, C.c_uint32]
    L.sim_zstd_parse_round.restype = C.c_uint32
    L.sim_zstd_parse_chunk_bytes.argtypes = [C.c_uint32]
    L.sim_zstd_parse_chunk_bytes.restype = C.c_uint64
    return L


def _load():
    global _S
    if _S is None:
        _S = load(build_so())
    return _S


def round_chunks(hw_buff_sz, nchunks):
    """chunks per scratch round of a call, from the host plan (qzd_zstd_parse_host.h)"""
    return _load().sim_zstd_parse_round(hw_buff_sz, nchunks)


def chunk_bytes(hw_buff_sz):
    return _load().sim_zstd_parse_chunk_bytes(hw_buff_sz)


def run(src, hw_buff_sz=65536, mini_match=3, flags=3, depth=16, round_cap=0, peek=False, records=False, lib=None):
    """-> (rc, stream, per-frame lengths, extras); extras: "chain", "res" (peek) and "seqs", "lits" (records), one chunk only.
    lib: a library from load(), the suite's own build otherwise"""
    L = lib or _load()
    n = len(src)
    nb = (n + hw_buff_sz - 1) // hw_buff_sz
    cap = zstd_format.bound(n, hw_buff_sz)
    out = C.create_string_buffer(cap + 64)
    ol = C.c_uint64(0)
    lens = (C.c_uint32 * max(nb, 1))()
    pk = np.zeros(3 * n, np.uint32) if peek else None
    sq = np.zeros(3 * (n // 3 + 1), np.uint32) if records else None
    lt = C.create_string_buffer(n + 16) if records else None
    cnt = (C.c_uint32 * 2)()
    rc = L.sim_zstd_parse(src, n, hw_buff_sz, mini_match, flags, depth, round_cap, out, cap, C.byref(ol), lens,
                          pk.ctypes.data if peek else None, sq.ctypes.data if records else None, lt, cnt)
    extra = {}
    if rc == 0 and peek:
        extra["chain"] = pk[:n].tolist()
        extra["res"] = [(int(a), int(b)) for a, b in pk[n:].reshape(-1, 2)]
    if rc == 0 and records:
        extra["seqs"] = [tuple(int(v) for v in r) for r in sq[:3 * cnt[0]].reshape(-1, 3)]
        extra["lits"] = lt.raw[:cnt[1]]
    return rc, out.raw[:ol.value], list(lens)[:nb], extra


def compress(src, hw_buff_sz=65536, mini_match=3, flags=3, depth=16, round_cap=0):
    """-> (stream of frames, per-frame lengths), as zstd_seq_sim.compress"""
    rc, stream, lens, _ = run(src, hw_buff_sz, mini_match, flags, depth, round_cap)
    assert rc == 0, "sim_zstd_parse rc=%d" % rc
    return stream, lens


def records(chunk, hw_buff_sz, mini_match=3, depth=16, flags=3, lib=None):
    """one chunk -> (its frame, [(ll, ml, off)], the literals)"""
    rc, stream, _, x = run(chunk, hw_buff_sz, mini_match, flags, depth, records=True, lib=lib)
    assert rc == 0
    return stream, x["seqs"], x["lits"]


def search(chunk, hw_buff_sz, mini_match, depth, lib=None):
    """one chunk -> (chain distances, [(length, distance)] per position)"""
    rc, _, _, x = run(chunk, hw_buff_sz, mini_match, 0, depth, peek=True, lib=lib)
    assert rc == 0
    return x["chain"], x["res"]


def index():
    with open(INDEX) as f:
        return json.load(f)


# ---------------------------------------------------------------- models
def match_len(b, p, q):
    """common prefix of b[p:] and b[q:], q < p"""
    a = np.frombuffer(b, np.uint8)
    n = len(b) - p
    ne = np.flatnonzero(a[p:] != a[q:q + n])
    return int(ne[0]) if len(ne) else n


def brute_longest(b, mm):
    """per position the longest match of at least mm bytes over all earlier positions, the nearest among equals"""
    out = []
    for p in range(len(b)):
        best = (0, 0)
        if p + mm <= len(b):
            key = b[p:p + mm]
            q = b.rfind(key, 0, p + mm - 1)
            while q >= 0:
                k = match_len(b, p, q)
                if k > best[0]:
                    best = (k, p - q)
                    if p + k == len(b):
                        break
                q = b.rfind(key, 0, q + mm - 1)
        out.append(best)
    return out


def check_sequences(chunk, seqs, mm, lits=None):
    """every record's match is mm bytes or more, starts 1 .. its position back, and copies what the chunk holds there; the
    literals (where given) are the chunk's.  -> the offsets"""
    p, lp, offs = 0, 0, []
    for ll, ml, off in seqs:
        if lits is not None:
            assert lits[lp:lp + ll] == chunk[p:p + ll]
        p += ll
        lp += ll
        assert ml >= mm and 1 <= off <= p, (ll, ml, off, p)
        assert p + ml <= len(chunk) and match_len(chunk, p, p - off) >= ml, (ll, ml, off, p)
        p += ml
        offs.append(off)
    if lits is not None:
        assert lits[lp:] == chunk[p:]
    return offs


# ---------------------------------------------------------------- inputs
def period(n, k, seed=5):
    r = random.Random(seed)
    unit = bytes(r.randrange(256) for _ in range(k))
    return (unit * (n // k + 1))[:n]


def small_inputs():
    """4096 bytes each: what the search is checked on against brute force"""
    return {"text": S.make_input("text", 4096, 3), "runs": S.make_input("runs", 4096, 3), "rand": S.make_input("rand", 4096, 3),
            "period3": period(4096, 3), "period200": period(4096, 200)}


def far_repeat():
    """128 KB whose second half repeats bytes 0 .. 59999 of the first at distance 70000; the rest does not repeat"""
    r = random.Random(77)
    b = bytearray(r.randrange(256) for _ in range(131072))
    b[70000:130000] = b[0:60000]
    return bytes(b)


def late_match(mm):
    """a match that begins in the last mm bytes of the chunk and nowhere earlier: text, then `abc`, a byte the text does not
    have, and `abc` again, so that the last mm bytes repeat at distance mm + 1 and the byte in front of them does not"""
    unit = b"abcd"[:mm]
    return S.make_input("text", 1500, 9).replace(b"\x01", b" ") + unit + b"\x01" + unit


def overlap():
    """distances below the lengths: runs of one byte and of a period of 5 between unrelated bytes"""
    r = random.Random(4)
    noise = lambda k: bytes(r.randrange(256) for _ in range(k))
    return noise(50) + b"Q" * 300 + noise(40) + b"abcde" * 80 + noise(34)


def rep_cases():
    """(name, chunk): `x, gap, x'` patterns where the match after a short gap continues at the offset of the match before
    it - the repeat offset.  gap 0: x with one byte deleted in the copy (ll == 0); gap > 0: one byte changed (ll > 0)."""
    r = random.Random(33)
    noise = lambda k: bytes(r.randrange(256) for _ in range(k))
    base = noise(600)
    changed = bytearray(base)
    changed[300] ^= 0x55                                   # copy with one byte changed: match, 1 literal, match at the SAME offset
    with_gap = noise(100) + base + noise(100) + bytes(changed) + noise(50)
    # ll == 0: the copy drops byte 300, so the second match starts at once, one byte farther in the source: its offset is the
    # first's less 1... which is rep1 - 1 only with ll == 0
    dropped = base[:300] + base[301:]
    no_gap = noise(100) + base + noise(100) + dropped + noise(50)
    return {"rep_ll_gt0": with_gap, "rep_ll0": no_gap}


def edge_cases():
    """name -> (input, hw_buff_sz, mini_match, depth): the smallest shapes that can go wrong, all pinned under flags 3"""
    E = {
        "hw1024_3073": (S.make_input("text", 3073, 11), 1024, 3, 16),          # four chunks, the last of 1 byte
        "tail1": (S.make_input("silesia", 4096 + 1, 11), 4096, 3, 4),
        "tail2": (S.make_input("silesia", 4096 + 2, 11), 4096, 4, 4),
        "tail3": (S.make_input("silesia", 4096 + 3, 11), 4096, 3, 64),
        "hw131072": (S.make_input("lzmix", 131072 + 777, 11), 131072, 3, 4),
        "all_one": (b"A" * 131072, 131072, 3, 4),
        "random": (S.make_input("rand", 5000, 11), 4096, 4, 64),
        "far": (far_repeat(), 131072, 3, 16),
        "late3": (late_match(3), 2048, 3, 16),
        "late4": (late_match(4), 2048, 4, 16),
        "overlap": (overlap(), 1024, 3, 16),
    }
    for k, v in rep_cases().items():
        E[k] = (v, 2048, 4, 16)
    for d in DEPTHS:
        E["depth%d" % d] = (S.make_input("lzmix", 20000, 11), 16384, 4, d)
    return E


KINDS = ("text", "records", "silesia", "lzmix", "runs", "mod200", "rand", "allA")      # gen_zstd_seq.py's, at 70001 bytes
RATIO_DEPTHS = (4, 16, 64)
LIBZSTD_LEVELS = (1, 3, 9)
