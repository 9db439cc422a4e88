"""The C-ABI library, built for gfx950 here (no GPU), exports what include/qzamd_zstd_parse.h declares and the device
layer's call with a parse depth; the headers beside it are untouched; qzstd-amd names --parse-depth and refuses 300."""
import ctypes
import os
import re
import subprocess

import test_cabi_exports as E


def test_library_exports_the_parse_call_and_the_device_call():
    import qatzip_amd
    L = ctypes.CDLL(qatzip_amd.build.build())
    assert E._declared("qzamd_zstd_parse.h") == ["qzSetSessionZstdParseAMD"]
    for n in ("qzSetSessionZstdParseAMD", "qzd_zstd_compress_frames_parse"):
        assert hasattr(L, n), "missing export: " + n
    assert {"qzd_zstd_compress_frames_parse", "qzd_zstd_compress_frames_ex", "qzd_zstd_compress_frames"} <= set(E._declared("qzamd_device.h"))
    # the older headers declare what they declared
    assert E._declared("qzamd_zstd.h") == ["qzSetupSessionZstdAMD"] and E._declared("qzamd_zstd_dec.h") == ["qzSetupSessionZstdDecAMD"]
    assert E._declared("qzamd_zstd_seq.h") == ["qzSetSessionZstdSeqAMD"]
    assert "qzSetSessionZstdParseAMD" not in E._declared("qatzip.h")


def test_the_header_is_in_the_build_list_and_defines_the_limit():
    import qatzip_amd.build as B
    assert any(s.endswith(os.path.join("include", "qzamd_zstd_parse.h")) for s in B._sources())
    txt = open(os.path.join(E.ROOT, "include", "qzamd_zstd_parse.h")).read()
    assert re.search(r"#define\s+QZ_ZSTD_PARSE_DEPTH_MAX\s+256u", txt)


def test_the_device_call_refuses_a_null_context():
    """all that can be asked without a device: QZD_ERR_PARAM for a NULL context under any depth.  The refusal of a depth above
    256 on a live context is tests/test_gpu_zstd_parse.py's, and the emulator driver's through the same qzd_zp_depth_ok"""
    import qatzip_amd
    L = ctypes.CDLL(qatzip_amd.build.build())
    for depth in (0, 16, 257):
        assert L.qzd_zstd_compress_frames_parse(None, None, 0, 65536, 3, 1, None, 0, None, None, 0, depth) == -1


def test_qzstd_amd_names_the_option_and_refuses_300(tmp_path):
    import qatzip_amd.build as B
    B.build()
    r = subprocess.run([B.ZSTD_CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--parse-depth" in r.stdout and "--seq-tables" in r.stdout
    f = tmp_path / "x.bin"
    f.write_bytes(b"abc" * 1000)
    for bad in ("300", "257", "-1", "x", ""):
        r = subprocess.run([B.ZSTD_CLI, "--parse-depth", bad, "-k", str(f)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--parse-depth" in r.stderr, (bad, r)
        assert f.exists() and not (tmp_path / "x.bin.zst").exists()


def test_the_python_device_layer_lists_the_call():
    from qatzip_amd import _lib
    assert "qzd_zstd_compress_frames_parse" in _lib.exported_symbols()
