"""Zstd sessions, the part that needs no GPU: qzSetupSessionZstdAMD (include/qzamd_zstd.h) checks what qzSetupSessionLZ4S
checks and refuses a hw_buff_sz above 128 KB and a callback on top of it; qzMaxCompressedLength of a zstd session against the
formula of INTEGRATION.md ("Zstd sessions")."""
import ctypes as C

import pytest

from qatzip_amd import api as A

import test_lz4s_params as P
import zstd_format


def _setup(cb=None, **kw):
    L = A.lib()
    s = A.QzSession()
    p = P._params(**kw)
    if cb is not None:
        p.qzCallback = cb
    rc = L.qzSetupSessionZstdAMD(C.byref(s), C.byref(p))
    if rc == A.QZ_OK:
        assert s.internal
        assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK
    else:
        assert not s.internal
    return rc


@pytest.mark.parametrize("kw", P.BAD + [dict(hw_buff_sz=256 * 1024), dict(hw_buff_sz=512 * 1024)], ids=str)
def test_refused(kw):
    assert _setup(**kw) == A.QZ_PARAMS


@pytest.mark.parametrize("kw", [g for g in P.GOOD if g.get("hw_buff_sz", 0) <= 128 * 1024] + [dict(hw_buff_sz=128 * 1024)], ids=str)
def test_accepted(kw):
    assert _setup(**kw) == A.QZ_OK


def test_a_callback_is_refused_and_null_arguments():
    cb = A.QzLZ4SCallback(lambda *a: 0)
    assert _setup(cb=cb) == A.QZ_PARAMS
    L = A.lib()
    p = P._params()
    assert L.qzSetupSessionZstdAMD(None, C.byref(p)) == A.QZ_PARAMS
    # NULL parameters: the current defaults, whose factory direction is QZ_DIR_BOTH - refused as qzSetupSessionLZ4S refuses them
    s = A.QzSession()
    assert L.qzSetupSessionZstdAMD(C.byref(s), None) == L.qzSetupSessionLZ4S(C.byref(A.QzSession()), None) == A.QZ_PARAMS


def test_duplicate_and_max_compressed_length():
    L = A.lib()
    s = A.QzSession()
    p = P._params(hw_buff_sz=4096)
    assert L.qzSetupSessionZstdAMD(C.byref(s), C.byref(p)) == A.QZ_OK
    assert L.qzSetupSessionZstdAMD(C.byref(s), C.byref(p)) == A.QZ_DUPLICATE
    for n in (1, 4095, 4096, 4097, 3 * 4096, 1000000):
        assert L.qzMaxCompressedLength(n, C.byref(s)) == zstd_format.bound(n, 4096) == n + 12 * ((n + 4095) // 4096)
    assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK
