"""The zstd kernels with seq_flags (include/qzamd_zstd_seq.h) on the CPU SIMT emulator, and what the tests of the option
share: used by tests/test_sim_zstd_seq.py, tests/test_gpu_zstd_seq.py and tests/golden/gen_zstd_seq.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import zstd_format
import zstd_full_format as F
import zstd_ref
import zstd_sim as S

SO = os.path.join(S.SIMDIR, "libqzsim_zstd_seq.so")
SRC = os.path.join(S.SIMDIR, "sim_zstd_seq.cpp")
INDEX = os.path.join(S.HERE, "golden", "zstd_seq", "index.json")
FSE_TABLES, REPEAT_OFFSETS = 1, 2

_S = None


def build_so():
    """g++ build of tests/sim/sim_zstd_seq.cpp, redone when a source is newer"""
    deps = [SRC] + [d for d in S._deps() if not d.endswith("sim_zstd.cpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-I", S.SIMDIR, "-Wno-unused-function",
                               "-o", SO, SRC])
    return SO


def _load():
    global _S
    if _S is None:
        L = C.CDLL(build_so())
        L.sim_zstd_ex.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                  C.POINTER(C.c_uint64), C.c_void_p, C.c_uint32]
        L.sim_zstd_encode_ex.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                         C.POINTER(C.c_uint64), C.c_void_p, C.c_uint32]
        _S = L
    return _S


def compress(src, hw_buff_sz=65536, mini_match=3, flags=3, waves=0):
    """-> (stream of frames, per-frame lengths), as zstd_sim.compress"""
    L = _load()
    n = len(src)
    nb = (n + hw_buff_sz - 1) // hw_buff_sz
    cap = zstd_format.bound(n, hw_buff_sz)
    out = C.create_string_buffer(cap + 64)
    ol = C.c_uint64(0)
    lens = (C.c_uint32 * max(nb, 1))()
    rc = L.sim_zstd_ex(src, n, hw_buff_sz, mini_match, waves, out, cap, C.byref(ol), lens, flags)
    assert rc == 0, "sim_zstd_ex rc=%d" % rc
    return out.raw[:ol.value], list(lens)[:nb]


def encode(frames, flags=3, waves=0):
    """the entropy stage alone -> (rc, stream, per-frame lengths), as zstd_sim.encode"""
    L = _load()
    lits, seqs, desc = S.pack_frames(frames)
    cap = sum(min(f[0], zstd_format.MAX_BLOCK) + 12 for f in frames)
    out = C.create_string_buffer(cap + 64)
    ol = C.c_uint64(0)
    lens = (C.c_uint32 * max(len(frames), 1))()
    seqs = np.concatenate([seqs, np.zeros(3, np.uint32)])
    rc = L.sim_zstd_encode_ex(lits + b"\0", seqs.ctypes.data, desc.ctypes.data, len(frames), waves, out, cap, C.byref(ol), lens, flags)
    return rc, out.raw[:ol.value], list(lens)[:len(frames)]


def index():
    with open(INDEX) as f:
        return json.load(f)


# ---------------------------------------------------------------- reading
def read_frame(buf, pos=0):
    """zstd_full_format.decode_frame, which keeps neither to itself: -> (info with "sequences", the lists its blocks held with
    repeat offsets resolved, and "logs", the accuracy of every table description read, in LL, OF, ML order; where the next
    frame begins)"""
    seqs, logs = [], []
    inner, ncount = F._sequences, F.read_ncount

    def spy(*a):
        r = inner(*a)
        seqs.extend(r)
        return r

    def spy_ncount(*a):
        r = ncount(*a)
        logs.append(r[1])
        return r
    F._sequences, F.read_ncount = spy, spy_ncount
    try:
        info, end = F.decode_frame(buf, pos)
    finally:
        F._sequences, F.read_ncount = inner, ncount
    info["sequences"], info["logs"] = seqs, logs
    return info, end


def read(stream, src, hw):
    """every frame of a stream by the strict reader and, where libzstd loads, ZSTD_decompress; -> the frames"""
    frames, pos = [], 0
    while pos < len(stream):
        f, pos = read_frame(stream, pos)
        frames.append(f)
    assert b"".join(f["data"] for f in frames) == src
    for i, f in enumerate(frames):
        assert f["content_size"] == min(hw, len(src) - i * hw)
        assert f["size"] <= f["content_size"] + 12
    zstd_ref.check(stream, src)
    return frames


def offset_values(seqs):
    """the model of the repeat-offset pass: the offset value of every (ll, ml, off), the lowest legal one, from the history
    1, 4, 8 (RFC 8878, 3.1.1.5); -> (values, the history afterwards)"""
    rep, out = [1, 4, 8], []
    for ll, _, off in seqs:
        cands = [rep[0], rep[1], rep[2]] if ll else [rep[1], rep[2], rep[0] - 1]
        if off in cands and off != 0:
            v = cands.index(off) + 1
        else:
            v = off + 3
        out.append(v)
        if v > 3:
            rep = [off, rep[0], rep[1]]
        else:
            idx = v - 1 + (0 if ll else 1)
            if idx == 1:
                rep = [off, rep[0], rep[2]]
            elif idx >= 2:
                rep = [off, rep[0], rep[1]]
    return out, rep


def rep_tally(seqs):
    """the "rep:..." entries zstd_full_format's tally holds for these records under QZ_ZSTD_SEQ_REPEAT_OFFSETS"""
    vals, _ = offset_values(seqs)
    return sorted(set("rep:%d:%s" % (v, "ll>0" if ll else "ll0") for v, (ll, _, _) in zip(vals, seqs) if v <= 3))


def modes(f):
    """{"ll": mode name, "of": ..., "ml": ...} from a frame's tally"""
    out = {}
    for t in f["tally"]:
        k, _, v = t.partition(":")
        if k in ("ll", "of", "ml"):
            out[k] = v
    return out


# ---------------------------------------------------------------- hand-made records
def frame_of(records, lit=lambda i: 65 + i % 23, head=0):
    """a frame from (ll, ml, off) records: `head` literals in front of the first record's own, literals by lit(i)"""
    records = list(records)
    if head:
        records[0] = (records[0][0] + head, records[0][1], records[0][2])
    nl = sum(r[0] for r in records)
    lits = bytes(lit(i) & 255 for i in range(nl))
    return (nl + sum(r[1] for r in records), records, lits)


LL_LOW = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048,
          4096, 8192, 16384, 32768, 65536]                          # the lowest literal length of each of the 36 codes
ML_LOW = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771,
                                65539]                              # the lowest match length of each of the 53 codes


def _edges():
    E = {}
    E["one"] = frame_of([(5, 300, 2)])
    E["two_ll"] = frame_of([(5, 150, 2), (20, 150, 2)])
    for n in (63, 64, 65, 127, 128):
        E["count%d" % n] = frame_of([(1 + i % 3, 3 + i % 5, 1 + i % 2) for i in range(n)])
    E["count7f00"] = S.many(0x7f00)
    E["skew"] = frame_of([(1, 4, 1)] * 299 + [(2, 9, 1)])          # one code ns - 1 times, another once
    E["ll_0_35"] = frame_of([(65536, 3, 1)] + [(0, 3 + i % 2, 1) for i in range(200)])
    E["ml_0_52"] = frame_of([(1, 65539, 1)] + [(1, 3, 1 + i % 2) for i in range(200)])
    return E


def all_ll():
    """One sequence per LL code does not exist: the lowest lengths of the 36 codes add up to 131376, with 36 matches of 3 to
    131484, above the 131072 a frame holds.  And with 36 sequences a description costs more than it saves, so that the
    accuracy would not show.  The nearest thing: every code but 34 (32768 .. 65535) once - 35 codes, code 35 among them -
    and 165 more sequences of code 0: 200 sequences ask for an accuracy of 5, 35 codes need 6."""
    return frame_of([(v, 3, 1) for v in LL_LOW[1:34]] + [(LL_LOW[35], 3, 1)] + [(0, 3, 1)] * 166)


def all_ml():
    """One sequence per ML code does not exist either: the lowest lengths of the 53 codes (3 .. 34, 35 37 39 41 43 47 51 59
    67 83 99 131 259 515 1027 2051 4099 8195 16387 32771 65539) add up to 132167.  The nearest thing: every code but 51
    (32771 .. 65538) once - 52 codes, code 52 among them, 99396 bytes of matches - and 148 more sequences of code 0: 200
    sequences ask for an accuracy of 5, 52 codes need 6."""
    return frame_of([(1, m, 1) for m in ML_LOW[:51]] + [(1, ML_LOW[52], 1)] + [(1, 3, 1)] * 148)


def uniform_of():
    """offsets whose codes (of offset + 3) are 2 .. 16, sixteen records each, rising so that the bytes are there to reach
    back into (a plain offset has no code below 2, and code 17 needs 131069 bytes in front of it); 500 literals a record"""
    recs, produced, k = [], 0, 0
    for code in range(2, 17):
        for _ in range(16):
            produced += 500
            low = max((1 << code) - 3, 1)
            span = min((1 << code) - 1, produced - low)
            assert span >= 0
            recs.append((500, 3, low + (k * 37) % (span + 1)))
            produced += 3
            k += 1
    return frame_of(recs, lit=lambda i: (i * 131 + (i >> 8)) & 255)


EDGES = _edges()
EDGES["all_ll"] = all_ll()
EDGES["all_ml"] = all_ml()
EDGES["uniform_of"] = uniform_of()

# repeat offsets
REP = {
    "first_1": frame_of([(9, 200, 1)]), "first_4": frame_of([(9, 200, 4)]), "first_8": frame_of([(9, 200, 8)]),
    # ll == 0 with rep2, rep3, rep1 - 1: after (9, 5, 6) the history is 6, 1, 4
    "ll0_rep2": frame_of([(9, 100, 6), (0, 100, 1)]), "ll0_rep3": frame_of([(9, 100, 6), (0, 100, 4)]), "ll0_rep1m1": frame_of([(9, 100, 6), (0, 100, 5)]),
    "ll0_rep1": frame_of([(9, 100, 6), (0, 100, 6)]),
    "all_a": (131072, [(1, 65535, 1), (0, 65532, 1), (0, 4, 1)], b"A"),
    "alternate": frame_of([(400, 5, 300)] + [(1 + i % 2, 4, 300 if i % 2 else 5) for i in range(400)]),
    # rep1 == 1 and ll == 0: rep1 - 1 is 0 and is no offset; the record's offset 9 is new
    "rep1_is_1": frame_of([(12, 100, 1), (0, 100, 9), (0, 100, 1)]),
}
