"""qzSetSessionZstdParseAMD (include/qzamd_zstd_parse.h), the part that needs no GPU: QZ_OK on a zstd session that
compresses, QZ_PARAMS for every other kind of session, for none, and for a depth above 256; independent of
qzSetSessionZstdSeqAMD in either order."""
import ctypes as C

import pytest

from qatzip_amd import api as A

from test_zstd_seq_params import _other, _zstd

GOOD = (0, 1, 256, 16, 0, 64)
BAD = (257, 0xffffffff)


@pytest.mark.parametrize("direction", (None, A.QZ_DIR_BOTH))
def test_accepted_on_a_zstd_session_that_compresses(direction):
    L = A.lib()
    s = _zstd(direction)
    for depth in GOOD:                                              # a new call replaces the value, 0 restores the default
        assert L.qzSetSessionZstdParseAMD(C.byref(s), depth) == A.QZ_OK
    for depth in BAD:
        assert L.qzSetSessionZstdParseAMD(C.byref(s), depth) == A.QZ_PARAMS
    # the bound is a Raw block's under every depth
    assert L.qzSetSessionZstdParseAMD(C.byref(s), 256) == A.QZ_OK
    assert L.qzMaxCompressedLength(100000, C.byref(s)) == 100000 + 12 * 7
    assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK
    assert L.qzSetSessionZstdParseAMD(C.byref(s), 16) == A.QZ_PARAMS    # torn down: not set up any more


@pytest.mark.parametrize("kind", ("lz4s", "lz4", "deflate", "deflate_ext"))
def test_refused_on_every_other_kind_of_session(kind):
    L = A.lib()
    s = _other(kind)
    for depth in (0, 1, 256, 257):
        assert L.qzSetSessionZstdParseAMD(C.byref(s), depth) == A.QZ_PARAMS
    assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK


def test_refused_on_a_decode_only_zstd_session_and_without_a_session():
    L = A.lib()
    s = _zstd(A.QZ_DIR_DECOMPRESS)
    for depth in (0, 16, 257):
        assert L.qzSetSessionZstdParseAMD(C.byref(s), depth) == A.QZ_PARAMS
    assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK
    assert L.qzSetSessionZstdParseAMD(None, 0) == A.QZ_PARAMS and L.qzSetSessionZstdParseAMD(None, 16) == A.QZ_PARAMS
    fresh = A.QzSession()
    assert L.qzSetSessionZstdParseAMD(C.byref(fresh), 16) == A.QZ_PARAMS and not fresh.internal


@pytest.mark.parametrize("first", ("seq", "parse"))
def test_the_two_setters_in_both_orders(first):
    """neither resets nor refuses the other: every value of each is accepted whatever the other holds, a refused value of
    one leaves both usable, and 0 of one is accepted while the other is set"""
    L = A.lib()
    s = _zstd()
    seq = lambda v: L.qzSetSessionZstdSeqAMD(C.byref(s), v)
    parse = lambda v: L.qzSetSessionZstdParseAMD(C.byref(s), v)
    a, b = (seq, parse) if first == "seq" else (parse, seq)
    top = {seq: 3, parse: 256}
    bad = {seq: 4, parse: 257}
    assert a(top[a]) == A.QZ_OK and b(top[b]) == A.QZ_OK
    assert a(bad[a]) == A.QZ_PARAMS and b(1) == A.QZ_OK and a(1) == A.QZ_OK
    assert b(bad[b]) == A.QZ_PARAMS and a(0) == A.QZ_OK and b(0) == A.QZ_OK
    assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK


def test_the_python_session_mirrors_the_call():
    s = A.Session(zstd=True, hw_buff_sz=16384)
    assert s.rc_setup == A.QZ_OK
    assert s.set_zstd_parse(16) == A.QZ_OK and s.set_zstd_parse(257) == A.QZ_PARAMS and s.set_zstd_parse(0) == A.QZ_OK
    assert s.set_zstd_seq(3) == A.QZ_OK and s.set_zstd_parse(256) == A.QZ_OK
    s.close()
