"""Zstd decoding on the GPU, all from committed fixtures (tests/golden/zstd_dec/, made by tests/golden/gen_zstd_dec.py where
libzstd loads): the device layer (qzd_zstd_decompress_frames) gives the bytes and the {status, in_used, out_len} the CPU
emulator pinned for the same kernels; zstd decode sessions (include/qzamd_zstd_dec.h) round-trip their own qzCompress output
and answer like an LZ4 session, situation by situation.  libzstd is required nowhere."""
import hashlib

import pytest

import zstd_sim as S
import zstdd_sim as D
import qatzip_amd
from qatzip_amd import api as A
from qatzip_amd._lib import zstd_bound

pytestmark = pytest.mark.gpu


def _sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def ctx():
    c = qatzip_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def idx():
    return D.index()


def device_decode(ctx, frames, caps):
    """the frames back to back, their outputs back to back -> ([(status, in_used, out_len)], [outputs])"""
    comp, segs, out_size = D.layout(frames, caps)
    d_in = ctx.alloc(len(comp) + 64); d_in.upload(comp)
    d_out = ctx.alloc(out_size + 64)
    res = ctx.zstd_decompress_frames(d_in, d_out, [tuple(int(x) for x in s) for s in segs])
    out = d_out.download(out_size).tobytes()
    d_in.free(); d_out.free()
    outs = [out[int(s["out_off"]):int(s["out_off"]) + int(r["out_len"])] for s, r in zip(segs, res)]
    return [(int(r["status"]), int(r["in_used"]), int(r["out_len"])) for r in res], outs


def test_every_committed_frame_in_one_call(ctx, idx):
    """(a)-(c) with the refusal frames mixed in between: the emulator's pinned results, the committed SHAs, and no
    refusal disturbs its neighbours"""
    good = [e for e in idx["frames"] if e["group"] != "d"]
    bad = [e for e in idx["frames"] if e["group"] == "d"]
    order = []
    for i, e in enumerate(good):
        order.append(e)
        if i < len(bad):
            order.append(bad[i])
    order += bad[len(good):]
    assert len(order) == len(idx["frames"]) >= 60
    res, outs = device_decode(ctx, [D.frame_bytes(e) for e in order], [e["content"] for e in order])
    for e, r, o in zip(order, res, outs):
        assert list(r) == e["sim"], (e["name"], r)
        if e["group"] != "d":
            assert r == (0, e["size"], e["content"]) and _sha(o) == e["sha256"], e["name"]
        else:
            assert r[0] != 0, e["name"]


def device_frames(ctx, src, hw, mm):
    d_src = ctx.alloc(max(len(src), 1)); d_src.upload(src)
    d_dst = ctx.alloc(zstd_bound(len(src), hw) + 64)
    n, lens = ctx.zstd_compress_frames(d_src, len(src), d_dst, hw, mm, 1, dst_cap=zstd_bound(len(src), hw))
    out = d_dst.download(n).tobytes()
    d_src.free(); d_dst.free()
    return out


@pytest.mark.parametrize("kind,n", [("text", 70001), ("silesia", 300000)])
def test_a_session_of_both_directions_round_trips(ctx, kind, n):
    """chunks of 1 KB, 4 KB, 64 KB and 128 KB, mini_match 3 and 4: the compressed bytes are a zstd session's (the device
    layer's frames, and the pins of tests/golden/zstd/index.json where a case is pinned), qzDecompress gives the input back"""
    src = S.make_input(kind, n, 11)
    pins = {(c["hw_buff_sz"], c["mini_match"]): c for c in S.index()["cases"] if (c["kind"], c["n"], c["seed"]) == (kind, n, 11)}
    assert pins
    for hw in (1024, 4096, 65536, 131072):
        for mm in (3, 4):
            s = A.Session(zstd_dec=A.QZ_DIR_BOTH, hw_buff_sz=hw, mini_match=mm)
            assert s.rc_setup == A.QZ_OK
            rc, used, comp, _ = s.compress(src, 1)
            assert (rc, used) == (A.QZ_OK, n)
            assert comp == device_frames(ctx, src, hw, mm), (hw, mm)
            if (hw, mm) in pins:
                assert (len(comp), _sha(comp)) == (pins[(hw, mm)]["out_len"], pins[(hw, mm)]["out_sha"])
            rc, used, out = s.decompress(comp, n)
            assert (rc, used) == (A.QZ_OK, len(comp)) and out == src, (hw, mm)
            s.close()


def _two(idx):
    by = {e["name"]: e for e in idx["frames"]}
    f1, f2 = D.frame_bytes(by["a_text_70001_L3_cs"]), D.frame_bytes(by["a_text_3073_L1"])
    return f1, f2, S.make_input("text", 70001, 11), S.make_input("text", 3073, 11)


def test_return_codes_are_an_lz4_sessions(idx):
    """first frame cut, second frame cut, dest too small for the first frame, dest holds the first frame but not the second,
    payload corrupt, empty source"""
    z1, z2, d1, d2 = _two(idx)
    l4 = A.Session(lz4=True)
    z = A.Session(zstd_dec=A.QZ_DIR_DECOMPRESS)
    assert l4.rc_setup == A.QZ_OK and z.rc_setup == A.QZ_OK
    rc, _, l1, _ = l4.compress(d1[:60000], 1)
    assert rc == A.QZ_OK
    rc, _, l2, _ = l4.compress(d2, 1)
    assert rc == A.QZ_OK
    d1l = d1[:60000]

    def both(zc, zcap, lc, lcap):
        a, b = z.decompress(zc, zcap), l4.decompress(lc, lcap)
        assert a[0] == b[0], (a[0], b[0])
        return a, b

    # both frames whole
    a, b = both(z1 + z2, len(d1) + len(d2), l1 + l2, len(d1l) + len(d2))
    assert a == (A.QZ_OK, len(z1) + len(z2), d1 + d2) and b == (A.QZ_OK, len(l1) + len(l2), d1l + d2)
    # first frame cut
    a, b = both(z1[:-1], len(d1), l1[:-1], len(d1l))
    assert a == (A.QZ_FAIL, 0, b"") and b == (A.QZ_FAIL, 0, b"")
    # second frame cut: the first one is delivered
    a, b = both(z1 + z2[:-1], len(d1) + len(d2), l1 + l2[:-1], len(d1l) + len(d2))
    assert a == (A.QZ_OK, len(z1), d1) and b == (A.QZ_OK, len(l1), d1l)
    # dest too small for the first frame
    a, b = both(z1 + z2, len(d1) - 1, l1 + l2, len(d1l) - 1)
    assert a == (A.QZ_BUF_ERROR, 0, b"") and b == (A.QZ_BUF_ERROR, 0, b"")
    # dest holds the first frame but not the second
    a, b = both(z1 + z2, len(d1) + len(d2) - 1, l1 + l2, len(d1l) + len(d2) - 1)
    assert a == (A.QZ_OK, len(z1), d1) and b == (A.QZ_OK, len(l1), d1l)
    # payload corrupt (both frames carry a content checksum)
    zc, lc = bytearray(z1), bytearray(l1)
    zc[len(zc) // 2] ^= 0x10; lc[len(lc) // 2] ^= 0x10
    a, b = both(bytes(zc) + z2, len(d1) + len(d2), bytes(lc) + l2, len(d1l) + len(d2))
    assert a == (A.QZ_FAIL, 0, b"") and b == (A.QZ_FAIL, 0, b"")
    # empty source
    a, b = both(b"", 100, b"", 100)
    assert a == (A.QZ_OK, 0, b"") and b == (A.QZ_OK, 0, b"")
    # the calls every LZ4s session refuses stay refused
    assert z.decompress_crc64(z1, len(d1))[0] == A.QZ_UNSUPPORTED_FMT
    z.close(); l4.close()


def test_a_frame_without_content_size_is_decoded_alone(idx):
    by = {e["name"]: e for e in idx["frames"]}
    e = by["a_lzmix_200000_L3_st"]
    assert not e["has_content"]
    f1, (_, f2, _, d2) = D.frame_bytes(e), _two(idx)
    d1 = S.make_input("lzmix", 200000, 11)
    skip = D.frame_bytes(by["c_skippable"])
    z = A.Session(zstd_dec=A.QZ_DIR_DECOMPRESS)
    assert z.rc_setup == A.QZ_OK
    stream = f2 + skip + f1 + f2
    rc, used, out = z.decompress(stream, 1 << 20)
    assert (rc, used) == (A.QZ_OK, len(f2) + len(skip) + len(f1)) and out == d2 + d1        # *src_len at its end
    rc, used, out = z.decompress(stream[used:], 1 << 20)
    assert (rc, used, out) == (A.QZ_OK, len(f2), d2)
    # the rest of dest is what it gets: one byte short of what it produces is a failure of the frame, as on an LZ4 session
    rc, used, out = z.decompress(f1, 200000 - 1)
    assert rc == A.QZ_FAIL
    rc, used, out = z.decompress(f1, 200000)
    assert (rc, used) == (A.QZ_OK, len(f1)) and out == d1
    z.close()
