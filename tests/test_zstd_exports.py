"""The C-ABI library, built for gfx950 here (no GPU), exports what include/qzamd_zstd.h declares, the device layer's zstd
calls, and qzstd-amd builds against the two headers."""
import ctypes
import os

import test_cabi_exports as E


def test_library_exports_the_zstd_session_and_device_calls():
    import qatzip_amd
    so = qatzip_amd.build.build()
    L = ctypes.CDLL(so)
    names = E._declared("qzamd_zstd.h")
    assert names == ["qzSetupSessionZstdAMD"]
    for n in names + ["qzd_zstd_bound", "qzd_zstd_compress_frames", "qzd_zstd_encode_frames"]:
        assert hasattr(L, n), "missing export: " + n
    assert set(["qzd_zstd_bound", "qzd_zstd_compress_frames", "qzd_zstd_encode_frames"]) <= set(E._declared("qzamd_device.h"))
    L.qzd_zstd_bound.restype = ctypes.c_uint64
    L.qzd_zstd_bound.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    assert L.qzd_zstd_bound(300000, 131072) == 300000 + 36 and L.qzd_zstd_bound(0, 65536) == 0


def test_qzstd_amd_is_built():
    import qatzip_amd.build as B
    B.build()
    assert os.access(B.ZSTD_CLI, os.X_OK)
