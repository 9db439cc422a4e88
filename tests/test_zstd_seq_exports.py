"""The C-ABI library, built for gfx950 here (no GPU), exports what include/qzamd_zstd_seq.h declares and the device layer's
_ex calls; the headers beside it are untouched; qzstd-amd names its two new options."""
import ctypes
import re
import subprocess

import test_cabi_exports as E


def test_library_exports_the_seq_call_and_the_ex_calls():
    import qatzip_amd
    so = qatzip_amd.build.build()
    L = ctypes.CDLL(so)
    assert E._declared("qzamd_zstd_seq.h") == ["qzSetSessionZstdSeqAMD"]
    for n in ("qzSetSessionZstdSeqAMD", "qzd_zstd_compress_frames_ex", "qzd_zstd_encode_frames_ex"):
        assert hasattr(L, n), "missing export: " + n
    assert {"qzd_zstd_compress_frames_ex", "qzd_zstd_encode_frames_ex", "qzd_zstd_compress_frames", "qzd_zstd_encode_frames"} <= set(E._declared("qzamd_device.h"))
    # the older headers declare what they declared
    assert E._declared("qzamd_zstd.h") == ["qzSetupSessionZstdAMD"] and E._declared("qzamd_zstd_dec.h") == ["qzSetupSessionZstdDecAMD"]
    assert "qzSetSessionZstdSeqAMD" not in E._declared("qatzip.h")


def test_the_header_defines_the_two_bits():
    import os
    txt = open(os.path.join(E.ROOT, "include", "qzamd_zstd_seq.h")).read()
    assert re.search(r"#define\s+QZ_ZSTD_SEQ_FSE_TABLES\s+1u", txt) and re.search(r"#define\s+QZ_ZSTD_SEQ_REPEAT_OFFSETS\s+2u", txt)


def test_the_ex_calls_refuse_a_bit_above_3_before_anything_else():
    """needs no device: the flags are checked with the other arguments, a NULL context first"""
    import qatzip_amd
    L = ctypes.CDLL(qatzip_amd.build.build())
    assert L.qzd_zstd_compress_frames_ex(None, None, 0, 65536, 3, 1, None, 0, None, None, 0) == -1
    assert L.qzd_zstd_encode_frames_ex(None, None, None, None, 0, None, 0, None, None, 0) == -1


def test_qzstd_amd_names_the_two_options():
    import qatzip_amd.build as B
    B.build()
    r = subprocess.run([B.ZSTD_CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--seq-tables" in r.stdout and "--repeat-offsets" in r.stdout and "--decompress" in r.stdout
