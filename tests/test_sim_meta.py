"""The kernels of block-addressable compression (qatzip_amd/csrc/qzk_meta.h) on the CPU SIMT emulator: the programmable
CRC against the bitwise model of tests/crcmodel.py, XXH32 of ranges against the oracle's, and the block plan / pack step
against a restatement in Python.  The -m gpu twin is tests/test_gpu_meta.py."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import crcmodel
import datagen
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)

RANGE_DT = np.dtype([("off", "<u8"), ("len", "<u4"), ("pad", "<u4")])
POS_DT = np.dtype([("offset", "<u8"), ("size", "<u4"), ("flags", "<u4")])
JOB_DT = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("len", "<u4"), ("pad", "<u4")])

CRC_LENS = (0, 1, 7, 8, 9, 255, 256, 257, 4095, 65536, 65537)


@pytest.fixture(scope="module")
def S():
    so = os.path.join(SIMDIR, "libqzsim_meta.so")
    deps = [os.path.join(SIMDIR, f) for f in ("sim_meta.cpp", "hipsim.h")]
    csrc = os.path.join(ROOT, "qatzip_amd", "csrc")
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-I", SIMDIR, "-Wno-unused-function",
                               "-o", so, os.path.join(SIMDIR, "sim_meta.cpp")])
    L = C.CDLL(so)
    L.sim_crcn.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                           C.c_uint64, C.c_void_p, C.c_void_p]
    L.sim_crcn.restype = None
    L.sim_xxh32_ranges.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.sim_xxh32_ranges.restype = None
    L.sim_blocks_pack.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                  C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.sim_blocks_pack.restype = None
    L.sim_blocks_unpack.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.sim_blocks_unpack.restype = None
    return L


def sim_crcn(S, data, ranges, cfg, start=None):
    ra = np.array([(o, n, 0) for o, n in ranges], dtype=RANGE_DT)
    out = np.zeros(len(ranges), np.uint64)
    st = None if start is None else np.array(start, np.uint64)
    S.sim_crcn(data, ra.ctypes.data, len(ranges), cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[5],
               None if st is None else st.ctypes.data, out.ctypes.data)
    return [int(v) for v in out]


@pytest.fixture(scope="module")
def buf():
    # text in front (structure), random bytes behind; the ranges below start at odd offsets of it
    return datagen.gen_bytes("text", 40000, 5) + datagen.gen_bytes("rand", 100000, 6)


def test_crcmodel_reproduces_the_catalogue():
    for name, (cfg, check) in crcmodel.CATALOGUE.items():
        assert crcmodel.crc(cfg, b"123456789") == check, name
        assert crcmodel.crc_fast(cfg, b"123456789") == check, name
        # chaining: the CRC of a message from the CRC of its first part
        assert crcmodel.crc(cfg, b"6789", start=crcmodel.crc(cfg, b"12345")) == check, name
        assert crcmodel.crc(cfg, b"", start=crcmodel.empty(cfg)) == crcmodel.empty(cfg), name
    assert crcmodel.crc(crcmodel.CRC32_ISO_HDLC, b"123456789") == zlib.crc32(b"123456789")
    blob = datagen.gen_bytes("rand", 3000, 2)
    for cfg, _ in crcmodel.CATALOGUE.values():
        assert crcmodel.crc_fast(cfg, blob, start=77) == crcmodel.crc(cfg, blob, start=77)


@pytest.mark.parametrize("name", sorted(crcmodel.CATALOGUE))
def test_crcn_kernel_matches_the_model(S, buf, name):
    cfg, check = crcmodel.CATALOGUE[name]
    assert sim_crcn(S, b"123456789", [(0, 9)], cfg) == [check]
    # every length at an odd start offset, all ranges in ONE launch
    ranges, off = [], 1
    for n in CRC_LENS:
        ranges.append((off, n))
        off = (off + n // 3 + 2) | 1
        assert off + max(CRC_LENS) <= len(buf)
    got = sim_crcn(S, buf, ranges, cfg)
    for (o, n), g in zip(ranges, got):
        assert g == crcmodel.crc_fast(cfg, buf[o:o + n]), (name, o, n)
    # a starting value: the CRC of what came before each range (here: the 1000 bytes in front of it, and for one range
    # nothing at all - the empty message's CRC)
    ranges = [(1001 + 2 * i, n) for i, n in enumerate(CRC_LENS)]
    start = [crcmodel.crc_fast(cfg, buf[o - 1000:o]) for o, _ in ranges]
    start[3] = crcmodel.empty(cfg)
    got = sim_crcn(S, buf, ranges, cfg, start)
    for i, ((o, n), g) in enumerate(zip(ranges, got)):
        want = crcmodel.crc_fast(cfg, buf[o:o + n]) if i == 3 else crcmodel.crc_fast(cfg, buf[o - 1000:o + n])
        assert g == want, (name, o, n)


def test_xxh32_ranges_kernel_matches_the_oracle(S, buf):
    lens = (0, 15, 16, 17, 2047, 2048, 65536)
    ranges, off = [], 3
    for n in lens:
        ranges.append((off, n))
        off += n // 2 + 5
    ra = np.array([(o, n, 0) for o, n in ranges], dtype=RANGE_DT)
    out = np.zeros(len(ranges), np.uint32)
    S.sim_xxh32_ranges(buf, ra.ctypes.data, len(ranges), out.ctypes.data)
    for (o, n), g in zip(ranges, out):
        piece = buf[o:o + n]
        assert int(g) == O.lib().qzo_xxh32(piece, len(piece), 0), (o, n)


def _plan(slot_len, n, B, thr):
    """the pack step restated: (offset, size, flag, bytes come from) per block"""
    out, off, soff = [], 0, 0
    for k, a in enumerate(slot_len):
        plain = min(B, n - k * B)
        keep = a <= thr
        size = a if keep else plain
        out.append((off, size, 1 if keep else 0, soff if keep else k * B))
        off += size
        soff += a
    return out, off


@pytest.mark.parametrize("nblocks", [1, 2, 65, 257, 1100])
def test_block_pack_against_a_restatement(S, nblocks):
    B, thr = 1024, 700
    n = (nblocks - 1) * B + 1                                   # a 1-byte last block
    plain = datagen.gen_bytes("rand", n, 40 + nblocks)
    rng = np.random.default_rng(nblocks)
    # stream lengths on both sides of the threshold, the threshold itself and one above included; odd lengths, so that
    # source and destination of the 16-byte copies sit at every alignment
    slot_len = rng.integers(1, 1400, nblocks).astype(np.uint32)
    slot_len[0] = thr
    if nblocks > 1:
        slot_len[1] = thr + 1
        slot_len[-1] = 3 if nblocks % 2 else 1200              # the last block kept (longer than its byte) or stored
    streams = datagen.gen_bytes("rand", int(slot_len.sum()), 90 + nblocks)
    want, total = _plan([int(a) for a in slot_len], n, B, thr)
    for cap in (total, total - 1, total // 2):
        dst = np.full(total + 64, 0xEE, np.uint8)
        pos = np.zeros(nblocks, POS_DT); inr = np.zeros(nblocks, RANGE_DT); outr = np.zeros(nblocks, RANGE_DT)
        tot = C.c_uint64(0)
        S.sim_blocks_pack(streams, slot_len.ctypes.data, plain, n, B, nblocks, thr, dst.ctypes.data, cap, pos.ctypes.data,
                          inr.ctypes.data, outr.ctypes.data, C.byref(tot))
        assert tot.value == total
        exp = np.full(total + 64, 0xEE, np.uint8)
        for k, (off, size, flag, frm) in enumerate(want):
            assert (int(pos[k]["offset"]), int(pos[k]["size"]), int(pos[k]["flags"])) == (off, size, flag), (nblocks, k)
            assert (int(inr[k]["off"]), int(inr[k]["len"])) == (k * B, min(B, n - k * B))
            fits = off + size <= cap
            assert (int(outr[k]["off"]), int(outr[k]["len"])) == (off, size if fits else 0), (nblocks, k, cap)
            if fits:
                exp[off:off + size] = np.frombuffer((streams if flag else plain)[frm:frm + size], np.uint8)
        assert (dst == exp).all(), (nblocks, cap)              # blocks that fit are there, nothing else was touched
        if cap == total:
            assert {f for _, _, f, _ in want} == ({0, 1} if nblocks > 1 else {1})


def test_block_unpack_copies_stored_blocks(S):
    comp = datagen.gen_bytes("rand", 9000, 7)
    jobs = np.array([(1, 0, 1024, 0), (1030, 2048, 1024, 0), (3001, 4096, 1, 0), (3003, 5120, 17, 0), (4000, 6144 + 5, 1000, 0)],
                    dtype=JOB_DT)
    out = np.full(8192, 0xEE, np.uint8)
    S.sim_blocks_unpack(comp, out.ctypes.data, jobs.ctypes.data, len(jobs))
    exp = np.full(8192, 0xEE, np.uint8)
    for j in jobs:
        exp[int(j["out_off"]):int(j["out_off"]) + int(j["len"])] = np.frombuffer(comp[int(j["in_off"]):int(j["in_off"]) + int(j["len"])], np.uint8)
    assert (out == exp).all()
