"""LZ4s sessions, the part that needs no GPU: qzSetupSessionLZ4S / qzSetDefaultsLZ4S check their parameters as the
reference's qzCheckParamsLZ4S does (src/qatzip_utils.c:604-635), the defaults round trip, QZ_DUPLICATE, and
qzMaxCompressedLength of an LZ4s session against the formula of INTEGRATION.md ("LZ4s sessions").

What touches the process-wide defaults runs in a child process: test_api_params.py reads them in this one."""
import ctypes as C
import os
import subprocess
import sys

from qatzip_amd import api as A

import lz4s_format

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(**kw):
    """valid LZ4s parameters, then the overrides: common fields by name, the three LZ4s fields by theirs"""
    L = A.lib()
    p = A.QzSessionParamsLZ4S()
    assert L.qzGetDefaultsLZ4S(C.byref(p)) == A.QZ_OK
    p.common_params.comp_algorithm = A.QZ_LZ4s
    p.common_params.direction = A.QZ_DIR_COMPRESS
    for k, v in kw.items():
        if k in ("lz4s_mini_match", "qzCallback_external"):
            setattr(p, k, v)
        else:
            setattr(p.common_params, k, v)
    return p


def _setup(**kw):
    L = A.lib()
    s = A.QzSession()
    p = _params(**kw)
    rc = L.qzSetupSessionLZ4S(C.byref(s), C.byref(p))
    if rc == A.QZ_OK:
        assert s.internal
        assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK
    else:
        assert not s.internal
    return rc


BAD = [dict(comp_algorithm=A.QZ_DEFLATE), dict(comp_algorithm=A.QZ_LZ4), dict(direction=A.QZ_DIR_DECOMPRESS),
       dict(direction=A.QZ_DIR_BOTH), dict(direction=3), dict(comp_lvl=0), dict(comp_lvl=13), dict(lz4s_mini_match=2),
       dict(lz4s_mini_match=5), dict(lz4s_mini_match=0),
       # the common fields every setup refuses (qzCheckParamsCommon)
       dict(sw_backup=2), dict(hw_buff_sz=0), dict(hw_buff_sz=1025), dict(hw_buff_sz=2 * 1024 * 1024), dict(strm_buff_sz=100),
       dict(input_sz_thrshold=100), dict(req_cnt_thrshold=0)]
GOOD = [dict(), dict(comp_lvl=1), dict(comp_lvl=12), dict(lz4s_mini_match=3), dict(lz4s_mini_match=4), dict(hw_buff_sz=1024),
        dict(hw_buff_sz=512 * 1024)]


def test_factory_defaults():
    L = A.lib()
    p = A.QzSessionParamsLZ4S()
    assert L.qzGetDefaultsLZ4S(C.byref(p)) == A.QZ_OK
    assert p.common_params.comp_algorithm == A.QZ_LZ4s and p.lz4s_mini_match == 3 and not p.qzCallback
    assert (p.common_params.hw_buff_sz, p.common_params.comp_lvl) == (65536, 1)
    assert L.qzGetDefaultsLZ4S(None) == A.QZ_PARAMS


def test_setup_checks_what_the_reference_checks():
    L = A.lib()
    assert L.qzSetupSessionLZ4S(None, None) == A.QZ_PARAMS
    for kw in BAD:
        assert _setup(**kw) == A.QZ_PARAMS, kw
    for kw in GOOD:
        assert _setup(**kw) == A.QZ_OK, kw
    # NULL parameters are the current defaults, checked like a caller's: the factory's direction is QZ_DIR_BOTH, which an
    # LZ4s session refuses - as in the reference (src/qatzip.c:1314-1321)
    s = A.QzSession()
    assert L.qzSetupSessionLZ4S(C.byref(s), None) == A.QZ_PARAMS and not s.internal


def test_duplicate_setup():
    L = A.lib()
    s = A.QzSession()
    p = _params()
    assert L.qzSetupSessionLZ4S(C.byref(s), C.byref(p)) == A.QZ_OK
    assert L.qzSetupSessionLZ4S(C.byref(s), C.byref(p)) == A.QZ_DUPLICATE
    assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK


def test_session_object_keeps_the_callback():
    seen = []

    def cb(ext, src, src_len, dest, dest_len, status):
        seen.append(1)
        return 0
    s = A.Session(lz4s=True, mini_match=4, callback=cb, comp_lvl=7)
    assert s.rc_setup == A.QZ_OK and isinstance(s.cb, A.QzLZ4SCallback)
    s.close()
    assert A.Session(lz4s=True, mini_match=5).rc_setup == A.QZ_PARAMS
    assert A.Session(lz4s=True, comp_lvl=13).rc_setup == A.QZ_PARAMS


def test_max_compressed_length_follows_the_formula():
    L = A.lib()
    for hw in (1024, 65536, 131072, 524288):
        s = A.Session(lz4s=True, hw_buff_sz=hw)
        assert s.rc_setup == A.QZ_OK
        for n in (1, 65535, 65536, 65537, 524288):
            exp = 0
            for pos in range(0, n, hw):
                c = min(hw, n - pos)
                exp += 4 + c + c // 255 + 4 * ((c + 65534) // 65535) + 16
            assert L.qzMaxCompressedLength(n, C.byref(s.s)) == exp == lz4s_format.bound(n, hw), (hw, n)
        assert L.qzMaxCompressedLength(0xffffffff, C.byref(s.s)) == 0      # does not fit 32 bits
        assert L.qzMaxCompressedLength(0, C.byref(s.s)) == 34
        s.close()
    # the other branches are what they were
    assert L.qzMaxCompressedLength(65536, None) == 73808
    s = A.Session(lz4=True)
    assert L.qzMaxCompressedLength(65536, C.byref(s.s)) == 65536 + 27 + 4 * 2 + 257
    s.close()


CHILD = r"""
import ctypes as C
from qatzip_amd import api as A
L = A.lib()
p = A.QzSessionParamsLZ4S(); L.qzGetDefaultsLZ4S(C.byref(p))
assert L.qzSetDefaultsLZ4S(None) == A.QZ_PARAMS
assert L.qzSetDefaultsLZ4S(C.byref(p)) == A.QZ_PARAMS                 # direction QZ_DIR_BOTH
p.common_params.direction = A.QZ_DIR_COMPRESS
for field, v in (("comp_algorithm", A.QZ_LZ4), ("direction", A.QZ_DIR_BOTH), ("comp_lvl", 0), ("comp_lvl", 13), ("hw_buff_sz", 1025),
                 ("sw_backup", 2)):
    old = getattr(p.common_params, field); setattr(p.common_params, field, v)
    assert L.qzSetDefaultsLZ4S(C.byref(p)) == A.QZ_PARAMS, field
    setattr(p.common_params, field, old)
for mm in (2, 5):
    p.lz4s_mini_match = mm
    assert L.qzSetDefaultsLZ4S(C.byref(p)) == A.QZ_PARAMS
q = A.QzSessionParamsLZ4S(); L.qzGetDefaultsLZ4S(C.byref(q))
assert q.lz4s_mini_match == 3 and q.common_params.direction == A.QZ_DIR_BOTH      # refused calls changed nothing
# what is set comes back
p.lz4s_mini_match = 4; p.common_params.comp_lvl = 9; p.common_params.hw_buff_sz = 131072; p.qzCallback_external = 0x1234
assert L.qzSetDefaultsLZ4S(C.byref(p)) == A.QZ_OK
L.qzGetDefaultsLZ4S(C.byref(q))
assert (q.lz4s_mini_match, q.common_params.comp_lvl, q.common_params.hw_buff_sz, q.qzCallback_external) == (4, 9, 131072, 0x1234)
assert (q.common_params.direction, q.common_params.comp_algorithm) == (A.QZ_DIR_COMPRESS, A.QZ_LZ4s)
# ... and NULL parameters now make an LZ4s session of them
s = A.QzSession()
assert L.qzSetupSessionLZ4S(C.byref(s), None) == A.QZ_OK
assert L.qzMaxCompressedLength(131072, C.byref(s)) == 4 + 131072 + 131072 // 255 + 4 * 3 + 16
assert L.qzTeardownSession(C.byref(s)) == A.QZ_OK
print("child ok")
"""


def test_defaults_round_trip_in_a_child_process():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
