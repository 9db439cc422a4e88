"""GPU parity for LZ4 sessions with comp_lvl 3-8 (LZ4-HC, qatzip_amd/csrc/qzk_lz4hc.h) through include/qatzip.h: byte for
byte the frames liblz4 1.9.3's LZ4F_compressFrame wrote for the same input and level (tests/golden/lz4hc, made by
tests/golden/gen_lz4hc.py with the library itself).  Levels 9-12 stay QZ_NOT_SUPPORTED; levels 1-2 are what they were.

qzCompressStream: the reference refuses every session that is not deflate raw / gzip-ext (src/qatzip_stream.c:477-483,
QZ_PARAMS) and so does this library, at every level - an LZ4 stream call has no bytes to compare; that contract is what is
checked here."""
import ctypes as C
import hashlib
import json
import os
import struct
import sys
import threading

import pytest

import datagen
import oracle_lib as O
from qatzip_amd import api as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "lz4hc")
sys.path.insert(0, os.path.join(HERE, "golden"))
with open(os.path.join(GOLD, "index.json")) as f:
    INDEX = json.load(f)


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _blocks(frame):
    """[(word, body offset)] of a frame with a 15-byte header"""
    pos, out = 15, []
    while True:
        w = struct.unpack_from("<I", frame, pos)[0]
        pos += 4
        if w == 0:
            return out, pos
        out.append((w, pos))
        pos += w & 0x7fffffff


@pytest.fixture(scope="module")
def sessions():
    ss = {}
    for lvl in (3, 4, 5, 6, 7, 8):
        ss[lvl] = A.Session(lz4=True, comp_lvl=lvl)
        assert ss[lvl].rc_setup == A.QZ_OK
    yield ss
    for s in ss.values():
        s.close()


def _check(s, src, c, what):
    rc, used, out, _ = s.compress(src, 1)
    assert rc == A.QZ_OK, (what, rc)
    assert used == len(src), what
    assert len(out) == c["out_len"] and _sha(out) == c["out_sha"], (what, len(out), c["out_len"])
    if "file" in c:
        with open(os.path.join(GOLD, c["file"]), "rb") as f:
            assert out == f.read(), what
    if len(src):
        rc, cused, back = s.decompress(out, len(src))
        assert rc == A.QZ_OK and cused == len(out) and back == src, (what, rc)
    return out


@pytest.mark.parametrize("kind", datagen.KINDS)
def test_every_index_case(sessions, kind):
    cases = [c for c in INDEX["cases"] if c["kind"] == kind]
    assert len(cases) == 14 * 6
    srcs = {}
    for c in cases:
        if c["n"] not in srcs:
            srcs[c["n"]] = datagen.gen_bytes(kind, c["n"], c["seed"])
            assert _sha(srcs[c["n"]]) == c["in_sha"]
        _check(sessions[c["level"]], srcs[c["n"]], c, (kind, c["n"], c["level"]))


def test_block_store_edges_and_whole_frames(sessions):
    import gen_lz4hc
    for e in INDEX["edge"]:
        src = gen_lz4hc.barely(e["seed"], e["n"])
        assert _sha(src) == e["in_sha"]
        out = _check(sessions[e["level"]], src, e, ("edge", e["n"], e["level"], e["outcome"]))
        assert [w for w, _ in _blocks(out)[0]] == e["words"]
    for fr in INDEX["files"]:
        src = datagen.gen_bytes(fr["kind"], fr["n"], fr["seed"])
        _check(sessions[fr["level"]], src, fr, fr["file"])


def test_compress_stream_answers_as_the_reference_does(sessions):
    """qzCompressStream on an LZ4 session: QZ_PARAMS and nothing consumed or produced, as before and as in the reference"""
    L = A.lib()
    src = datagen.gen_bytes("text", 65536, 41)
    for lvl in (3, 6, 8):
        strm = A.QzStream()
        ibuf = C.create_string_buffer(src, len(src)); obuf = C.create_string_buffer(1 << 17)
        strm.in_ = C.cast(ibuf, C.c_void_p); strm.in_sz = len(src)
        strm.out = C.cast(obuf, C.c_void_p); strm.out_sz = len(obuf)
        assert L.qzCompressStream(C.byref(sessions[lvl].s), C.byref(strm), 1) == A.QZ_PARAMS
        assert strm.in_sz == 0 and strm.out_sz == 0


def test_compress2_and_crc_routes(sessions):
    """the same bytes through qzCompress2 (queued, with a callback) and qzCompressCrc"""
    L = A.lib()
    picks = [c for c in INDEX["cases"] if c["kind"] in ("text", "silesia") and c["n"] in (4000, 65536, 200777) and c["level"] in (3, 6, 8)]
    assert len(picks) == 18
    srcs = [datagen.gen_bytes(c["kind"], c["n"], c["seed"]) for c in picks]
    bufs_in = [C.create_string_buffer(x, len(x)) for x in srcs]
    bufs_out = [C.create_string_buffer(len(x) + 4096) for x in srcs]
    results = [A.QzResult() for _ in srcs]
    done, order = threading.Event(), []

    def on_done(res):
        order.append(res.contents.cb_tag)
        if len(order) == len(srcs):
            done.set()
        return 0
    cb = A.QzAsyncCallback(on_done)
    for i, c in enumerate(picks):
        results[i].cb_tag = i + 1; results[i].src_len = len(srcs[i]); results[i].dest_len = len(bufs_out[i])
        assert L.qzCompress2(C.byref(sessions[c["level"]].s), bufs_in[i], bufs_out[i], cb, C.byref(results[i])) == A.QZ_OK
    assert done.wait(300)
    for i, c in enumerate(picks):
        r = results[i]
        assert r.status == A.QZ_OK and r.src_len == c["n"] and r.dest_len == c["out_len"], (i, r.status)
        assert _sha(bufs_out[i].raw[:r.dest_len]) == c["out_sha"], (c["kind"], c["n"], c["level"])
        rc, used, out, _ = sessions[c["level"]].compress(srcs[i], 1, crc0=0)
        assert rc == A.QZ_OK and used == c["n"] and _sha(out) == c["out_sha"]


def test_eight_threads_at_mixed_levels():
    """64 KB calls of eight threads at once, levels 1, 3, 6 and 8 mixed: every caller gets its own level's frame"""
    by = {(c["kind"], c["level"]): c for c in INDEX["cases"] if c["n"] == 65536}
    errs, start = [], threading.Barrier(8)

    def body(t):
        try:
            ss = {lvl: A.Session(lz4=True, comp_lvl=lvl) for lvl in (1, 3, 6, 8)}
            kinds = [datagen.KINDS[(t + j) % len(datagen.KINDS)] for j in range(3)]
            srcs = {k: datagen.gen_bytes(k, 65536, 41) for k in kinds}
            ss[1].compress(b"warm up the session", 1)
            start.wait()
            for i in range(12):
                lvl = (1, 3, 6, 8)[(t + i) % 4]
                k = kinds[i % 3]
                rc, used, out, _ = ss[lvl].compress(srcs[k], 1)
                assert rc == A.QZ_OK and used == 65536, (t, i, lvl, rc)
                if lvl == 1:
                    assert out == O.sw_compress("LZ4", srcs[k], 65536, 1, cap=70000)[2], (t, i, k)
                else:
                    c = by[(k, lvl)]
                    assert len(out) == c["out_len"] and _sha(out) == c["out_sha"], (t, i, k, lvl)
            for s in ss.values():
                s.close()
        except Exception as e:   # noqa: BLE001
            errs.append((t, repr(e)))
    th = [threading.Thread(target=body, args=(t,)) for t in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join(900)
    assert not errs, errs


def test_hardware_path_framing():
    """qzamd_set_hw_framing at hw_buff_sz 64 KB and 256 KB: a frame per chunk behind qzLZ4HeaderGen's header (checked as
    tests/test_gpu_lz4.py checks it), then exactly what liblz4 wrote behind its own header for that chunk at that level"""
    L = A.lib()
    L.qzamd_set_hw_framing.argtypes = [C.c_void_p, C.c_int]
    assert {h["hw_buff_sz"] for h in INDEX["hw"]} == {65536, 262144} and len(INDEX["hw"]) == 24
    for h in INDEX["hw"]:
        hw = h["hw_buff_sz"]
        s = A.Session(lz4=True, hw_buff_sz=hw, comp_lvl=h["level"])
        assert s.rc_setup == A.QZ_OK and L.qzamd_set_hw_framing(C.byref(s.s), 1) == A.QZ_OK
        src = datagen.gen_bytes(h["kind"], h["n"], h["seed"])
        assert _sha(src) == h["in_sha"]
        rc, used, out, _ = s.compress(src, 1)
        what = (h["kind"], h["n"], hw, h["level"])
        assert rc == A.QZ_OK and used == h["n"], (what, rc)
        pos = 0
        for i, ch in enumerate(h["chunks"]):
            piece = src[i * hw:(i + 1) * hw]
            desc = bytes([0x4C, 0x40]) + len(piece).to_bytes(8, "little")
            hdr = bytes([0x04, 0x22, 0x4D, 0x18]) + desc + bytes([(O.lib().qzo_xxh32(desc, len(desc), 0) >> 8) & 0xff])
            assert out[pos:pos + 15] == hdr, (what, i)
            body = out[pos + 15:pos + 15 + ch["len"]]
            assert len(body) == ch["len"] and _sha(body) == ch["sha"], (what, i)
            pos += 15 + ch["len"]
        assert pos == len(out), what
        rc, cused, back = s.decompress(out, h["n"] + 64)
        assert rc == A.QZ_OK and back == src and cused == len(out), what
        s.close()


def test_one_call_of_256_mib_at_level_6():
    """one linked frame of 4096 blocks, each parsed by a wave of its own: total length, 64 blocks at fixed places against
    the same blocks of liblz4's frame, and the way back"""
    big = INDEX["big"]
    assert len(big["blocks"]) == 64
    src = datagen.gen_bytes(big["kind"], big["n"], big["seed"])
    assert _sha(src) == big["in_sha"]
    s = A.Session(lz4=True, comp_lvl=big["level"])
    rc, used, out, _ = s.compress(src, 1)
    assert rc == A.QZ_OK and used == big["n"], rc
    assert len(out) == big["out_len"], (len(out), big["out_len"])
    assert out[4] == 0x4C
    blocks, end = _blocks(out)
    assert len(blocks) == 4096 and end + 4 == len(out)
    for b in big["blocks"]:
        w, at = blocks[b["index"]]
        assert w == b["word"], (b["index"], w, b["word"])
        assert _sha(out[at:at + (w & 0x7fffffff)]) == b["sha"], b["index"]
    rc, cused, back = s.decompress(out, big["n"])
    assert rc == A.QZ_OK and cused == len(out) and back == src
    s.close()


@pytest.mark.parametrize("lvl", [9, 10, 12])
def test_levels_above_8_are_not_supported(lvl):
    s = A.Session(lz4=True, comp_lvl=lvl)
    assert s.rc_setup == A.QZ_OK
    for n in (1000, 65536, 200000):
        src = datagen.gen_bytes("text", n, 3)
        cap = n + 4096
        sl, dl = C.c_uint(n), C.c_uint(cap)
        dst = C.create_string_buffer(b"\xa5" * cap, cap)
        rc = s.L.qzCompress(C.byref(s.s), src, C.byref(sl), dst, C.byref(dl), 1)
        assert rc == A.QZ_NOT_SUPPORTED and sl.value == 0 and dl.value == 0
        assert dst.raw == b"\xa5" * cap                             # nothing written
    s.close()


def test_level_2_is_still_level_1():
    s = A.Session(lz4=True, comp_lvl=2)
    for kind, n in (("text", 65536), ("silesia", 40000), ("runs", 1000)):
        src = datagen.gen_bytes(kind, n, 5)
        rc, used, out, _ = s.compress(src, 1, cap=n + 200)
        assert rc == A.QZ_OK and used == n and out == O.sw_compress("LZ4", src, 65536, 1, cap=n + 200)[2]
    with open(os.path.join(HERE, "golden", "lz4_linked", "index.json")) as f:
        linked = json.load(f)["frames"]
    for fr in linked[:3]:
        src = datagen.gen_bytes(fr["kind"], fr["n"], fr["seed"])
        rc, used, out, _ = s.compress(src, 1)
        with open(os.path.join(HERE, "golden", "lz4_linked", fr["file"]), "rb") as f:
            assert rc == A.QZ_OK and out == f.read(), fr["file"]
    s.close()
