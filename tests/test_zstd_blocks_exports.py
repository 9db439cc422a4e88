"""The block route of the zstd decoder, the part that needs no GPU: the library built for gfx950 here exports what
include/qzamd_zstd_blocks.h declares, the calls check their parameters before they touch a device, a call without counts is
the call that has none, and the session call refuses what is no zstd decode session."""
import ctypes as C

from qatzip_amd import api as A
from qatzip_amd import _lib

import test_cabi_exports as E

NAMES = ["qzSetSessionZstdDecodeRouteAMD", "qzd_zstd_count_blocks", "qzd_zstd_decode_route", "qzd_zstd_decompress_frames_ex"]


def _lib_c():
    import qatzip_amd
    return C.CDLL(qatzip_amd.build.build())


def test_library_exports_what_the_header_declares():
    L = _lib_c()
    assert E._declared("qzamd_zstd_blocks.h") == NAMES
    for n in NAMES:
        assert hasattr(L, n), "missing export: " + n
    for n in NAMES[1:]:
        assert n in _lib.exported_symbols()
    # the older call and its header stay
    assert hasattr(L, "qzd_zstd_decompress_frames") and "qzd_zstd_decompress_frames" in E._declared("qzamd_device.h")
    assert "qzd_zstd_decompress_frames_ex" not in E._declared("qzamd_device.h")


def test_parameter_refusals_need_no_device():
    L = _lib_c()
    vp = C.c_void_p
    L.qzd_zstd_decompress_frames_ex.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp]
    L.qzd_zstd_decompress_frames.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]
    L.qzd_zstd_count_blocks.argtypes = [vp, vp, vp, C.c_uint32, vp]
    L.qzd_zstd_decode_route.argtypes = [vp, C.c_int]
    buf = C.create_string_buffer(64)
    counts = (C.c_uint32 * 4)(1, 2, 3, 4)
    PARAM = -1
    # a NULL context: with and without counts, as the call without counts answers
    for nb in (None, counts):
        assert L.qzd_zstd_decompress_frames_ex(None, buf, buf, buf, 1, buf, nb) == PARAM
    assert L.qzd_zstd_decompress_frames(None, buf, buf, buf, 1, buf) == PARAM
    assert L.qzd_zstd_count_blocks(None, buf, buf, 1, counts) == PARAM
    for r in (0, 1, 2, 3, -1):
        assert L.qzd_zstd_decode_route(None, r) == PARAM


def test_the_session_call_checks_its_session():
    L = A.lib()
    assert L.qzSetSessionZstdDecodeRouteAMD(None, 0) == A.QZ_PARAMS
    s = A.QzSession()
    assert L.qzSetSessionZstdDecodeRouteAMD(C.byref(s), 0) == A.QZ_PARAMS            # not set up
    assert "zstd_decode_route" in dir(A.Session) and "zstd_decode_route" in dir(_lib.Context)
    assert _lib.Context.ZSTDD_ROUTES == A.Session.ZSTDD_ROUTES == {"auto": 0, "frame": 1, "blocks": 2}
