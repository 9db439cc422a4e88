"""Zstd decode sessions, the part that needs no GPU: the library built for gfx950 here exports what
include/qzamd_zstd_dec.h declares and the device layer's qzd_zstd_decompress_frames, qzstd-amd builds against the headers
and knows --decompress, and qzSetupSessionZstdDecAMD checks its parameters before it touches a device."""
import ctypes as C
import os
import subprocess

from qatzip_amd import api as A

import test_cabi_exports as E
import test_lz4s_params as P


def test_library_exports_the_decode_session_and_device_call():
    import qatzip_amd
    so = qatzip_amd.build.build()
    L = C.CDLL(so)
    assert E._declared("qzamd_zstd_dec.h") == ["qzSetupSessionZstdDecAMD"]
    assert E._declared("qzamd_zstd.h") == ["qzSetupSessionZstdAMD"]
    for n in ("qzSetupSessionZstdDecAMD", "qzd_zstd_decompress_frames"):
        assert hasattr(L, n), "missing export: " + n
    assert "qzd_zstd_decompress_frames" in E._declared("qzamd_device.h")


def test_qzstd_amd_is_built_and_names_the_long_option():
    import qatzip_amd.build as B
    B.build()
    assert os.access(B.ZSTD_CLI, os.X_OK)
    r = subprocess.run([B.ZSTD_CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--decompress" in r.stdout and "-C <bytes>" in r.stdout
    # no device is needed for these answers
    r = subprocess.run([B.ZSTD_CLI, "--decompress", "no_suffix"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "-o" in r.stderr
    r = subprocess.run([B.ZSTD_CLI, "-d", "x.zst"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "zstd -d" in r.stderr


def _setup(direction, cb=None, **kw):
    L = A.lib()
    s = A.QzSession()
    p = P._params(**kw)
    p.common_params.direction = direction
    if cb is not None:
        p.qzCallback = cb
    rc = L.qzSetupSessionZstdDecAMD(C.byref(s), C.byref(p))
    if rc == A.QZ_OK:
        assert s.internal
        assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK
    else:
        assert not s.internal
    return rc


def test_setup_checks():
    assert _setup(A.QZ_DIR_COMPRESS) == A.QZ_PARAMS                  # qzSetupSessionZstdAMD is that session
    for d in (A.QZ_DIR_DECOMPRESS, A.QZ_DIR_BOTH):
        assert _setup(d) == A.QZ_OK
        assert _setup(d, hw_buff_sz=128 * 1024) == A.QZ_OK
        assert _setup(d, hw_buff_sz=256 * 1024) == A.QZ_PARAMS
        assert _setup(d, cb=A.QzLZ4SCallback(lambda *a: 0)) == A.QZ_PARAMS
        for kw in P.BAD:
            if "direction" not in kw:
                assert _setup(d, **kw) == A.QZ_PARAMS, kw
    assert _setup(3) == A.QZ_PARAMS
    L = A.lib()
    assert L.qzSetupSessionZstdDecAMD(None, C.byref(P._params())) == A.QZ_PARAMS
    # NULL parameters: the current LZ4s defaults, whose factory direction is QZ_DIR_BOTH
    s = A.QzSession()
    assert L.qzSetupSessionZstdDecAMD(C.byref(s), None) == A.QZ_OK
    assert L.qzSetupSessionZstdDecAMD(C.byref(s), None) == A.QZ_DUPLICATE
    assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK
