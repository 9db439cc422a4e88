"""qzSetSessionZstdSeqAMD (include/qzamd_zstd_seq.h), the part that needs no GPU: QZ_OK on a zstd session that compresses,
QZ_PARAMS for every other kind of session, for none, and for a bit other than the two."""
import ctypes as C

import pytest

from qatzip_amd import api as A

import test_lz4s_params as P


def _zstd(direction=None):
    L = A.lib()
    s = A.QzSession()
    p = P._params(hw_buff_sz=16384)
    if direction is None:
        assert L.qzSetupSessionZstdAMD(C.byref(s), C.byref(p)) == A.QZ_OK
    else:
        p.common_params.direction = direction
        assert L.qzSetupSessionZstdDecAMD(C.byref(s), C.byref(p)) == A.QZ_OK
    return s


def _other(kind):
    L = A.lib()
    s = A.QzSession()
    if kind == "lz4s":
        p = P._params()
        assert L.qzSetupSessionLZ4S(C.byref(s), C.byref(p)) == A.QZ_OK
    elif kind == "lz4":
        p = A.QzSessionParamsLZ4(); L.qzGetDefaultsLZ4(C.byref(p))
        p.common_params.comp_algorithm = A.QZ_LZ4
        assert L.qzSetupSessionLZ4(C.byref(s), C.byref(p)) == A.QZ_OK
    elif kind == "deflate":
        p = A.QzSessionParams(); L.qzGetDefaults(C.byref(p))
        assert L.qzSetupSession(C.byref(s), C.byref(p)) == A.QZ_OK
    else:
        p = A.QzSessionParamsDeflateExt(); L.qzGetDefaultsDeflateExt(C.byref(p))
        p.deflate_params.data_fmt = A.QZ_DEFLATE_RAW; p.zlib_format = 1
        assert L.qzSetupSessionDeflateExt(C.byref(s), C.byref(p)) == A.QZ_OK
    return s


@pytest.mark.parametrize("direction", (None, A.QZ_DIR_BOTH))
def test_accepted_on_a_zstd_session_that_compresses(direction):
    L = A.lib()
    s = _zstd(direction)
    for flags in (0, 1, 2, 3, 0, 3):                                # a new call replaces the setting, 0 restores the old writer
        assert L.qzSetSessionZstdSeqAMD(C.byref(s), flags) == A.QZ_OK
    for flags in (4, 5, 7, 8, 0x80000000, 0xffffffff):
        assert L.qzSetSessionZstdSeqAMD(C.byref(s), flags) == A.QZ_PARAMS
    # the bound is a Raw block's under every setting
    assert L.qzMaxCompressedLength(100000, C.byref(s)) == 100000 + 12 * 7
    assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK
    assert L.qzSetSessionZstdSeqAMD(C.byref(s), 3) == A.QZ_PARAMS   # torn down: not set up any more


@pytest.mark.parametrize("kind", ("lz4s", "lz4", "deflate", "deflate_ext"))
def test_refused_on_every_other_kind_of_session(kind):
    L = A.lib()
    s = _other(kind)
    for flags in (0, 3, 4):
        assert L.qzSetSessionZstdSeqAMD(C.byref(s), flags) == A.QZ_PARAMS
    assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK


def test_refused_on_a_decode_only_zstd_session_and_without_a_session():
    L = A.lib()
    s = _zstd(A.QZ_DIR_DECOMPRESS)
    for flags in (0, 3, 4):
        assert L.qzSetSessionZstdSeqAMD(C.byref(s), flags) == A.QZ_PARAMS
    assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK
    assert L.qzSetSessionZstdSeqAMD(None, 0) == A.QZ_PARAMS and L.qzSetSessionZstdSeqAMD(None, 3) == A.QZ_PARAMS
    fresh = A.QzSession()
    assert L.qzSetSessionZstdSeqAMD(C.byref(fresh), 3) == A.QZ_PARAMS and not fresh.internal


def test_the_python_session_mirrors_the_call():
    s = A.Session(zstd=True, hw_buff_sz=16384)
    assert s.rc_setup == A.QZ_OK
    assert s.set_zstd_seq(A.QZ_ZSTD_SEQ_FSE_TABLES | A.QZ_ZSTD_SEQ_REPEAT_OFFSETS) == A.QZ_OK and s.set_zstd_seq(4) == A.QZ_PARAMS
    s.close()
    assert (A.QZ_ZSTD_SEQ_FSE_TABLES, A.QZ_ZSTD_SEQ_REPEAT_OFFSETS) == (1, 2)
