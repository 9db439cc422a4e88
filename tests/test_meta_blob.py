"""Metadata blobs and CRC configs of include/qatzip.h, the parts that need no device: the parameter rules of
qzAllocateMetadata / qzFreeMetadata / qzMetadataBlockRead / Write / GetCrc32 / GetCrc64 and of the session CRC configs.
The blob code lives in qz_api.cpp and touches no GPU, so the library as built here serves."""
import ctypes as C

import pytest

import crcmodel
from qatzip_amd import api as A


@pytest.fixture(scope="module")
def L():
    return A.lib()


def test_allocate_parameter_rules(L):
    h = C.c_void_p()
    assert L.qzAllocateMetadata(None, 65536, 65536) == A.QZ_PARAMS
    assert L.qzAllocateMetadata(C.byref(h), 0, 65536) == A.QZ_PARAMS
    assert L.qzAllocateMetadata(C.byref(h), (1 << 30) + 1, 65536) == A.QZ_PARAMS
    for bad in (0, 512, 1000, 3 * 1024, 65536 + 1, 1024 * 1024):      # what qzSetupSession refuses as hw_buff_sz
        assert L.qzAllocateMetadata(C.byref(h), 65536, bad) == A.QZ_PARAMS, bad
    assert not h.value
    for good in (1024, 65536, 512 * 1024):
        m = A.Metadata(1 << 30, good)
        assert m.rc_alloc == A.QZ_OK and m.h.value
        assert m.read((1 << 30) // good - 1)[0] == A.QZ_OK and m.read((1 << 30) // good)[0] == A.QZ_OUT_OF_RANGE
        assert m.free() == A.QZ_OK


def test_block_count_is_rounded_up_and_records_start_zeroed():
    m = A.Metadata(3 * 1024 + 1, 1024)
    assert m.rc_alloc == A.QZ_OK
    for k in range(4):
        assert m.read(k) == (A.QZ_OK, 0, 0, 0, 0)
        assert m.crc32(k) == (A.QZ_OK, 0, 0) and m.crc64(k) == (A.QZ_OK, 0, 0)
    assert m.read(4)[0] == A.QZ_OUT_OF_RANGE and m.write(4, 1, 1, 1, 1) == A.QZ_OUT_OF_RANGE
    assert m.crc32(4)[0] == A.QZ_OUT_OF_RANGE and m.crc64(4)[0] == A.QZ_OUT_OF_RANGE
    assert m.free() == A.QZ_OK


def test_null_and_foreign_blobs_are_refused(L):
    v = C.c_uint32(0); w = C.c_uint64(0)
    junk = C.create_string_buffer(256)
    for blob in (None, C.cast(junk, C.c_void_p)):
        assert L.qzFreeMetadata(blob) == A.QZ_PARAMS
        assert L.qzMetadataBlockRead(0, blob, C.byref(v), None, None, None) == A.QZ_PARAMS
        assert L.qzMetadataBlockWrite(0, blob, C.byref(v), None, None, None) == A.QZ_PARAMS
        assert L.qzMetadataBlockGetCrc32(0, blob, C.byref(v), None) == A.QZ_PARAMS
        assert L.qzMetadataBlockGetCrc64(0, blob, C.byref(w), None) == A.QZ_PARAMS


def test_write_skips_null_fields_and_read_skips_null_outputs(L):
    m = A.Metadata(4096, 1024)
    assert m.write(2, offset=100, size=200, flags=1, hash=0xDEADBEEF) == A.QZ_OK
    assert m.read(2) == (A.QZ_OK, 100, 200, 1, 0xDEADBEEF)
    assert m.write(2, size=7) == A.QZ_OK                           # the other three are passed as NULL
    assert m.read(2) == (A.QZ_OK, 100, 7, 1, 0xDEADBEEF)
    assert m.write(2, flags=0, hash=5) == A.QZ_OK
    assert m.read(2) == (A.QZ_OK, 100, 7, 0, 5)
    assert m.write(2) == A.QZ_OK                                   # all NULL: nothing changes
    assert m.read(2) == (A.QZ_OK, 100, 7, 0, 5)
    assert m.read(1) == (A.QZ_OK, 0, 0, 0, 0) and m.read(3) == (A.QZ_OK, 0, 0, 0, 0)
    z = C.c_uint32(9)
    assert L.qzMetadataBlockRead(2, m.h, None, C.byref(z), None, None) == A.QZ_OK and z.value == 7
    assert L.qzMetadataBlockRead(2, m.h, None, None, None, None) == A.QZ_OK
    assert L.qzMetadataBlockGetCrc32(2, m.h, None, None) == A.QZ_OK
    # a written record still passes its check: the write refreshed the word
    assert m.crc32(2) == (A.QZ_OK, 0, 0) and m.crc64(2) == (A.QZ_OK, 0, 0)
    assert m.free() == A.QZ_OK


def test_a_corrupted_record_fails_its_check_word():
    m = A.Metadata(4096, 1024)
    assert m.write(1, offset=10, size=20, flags=1, hash=30) == A.QZ_OK
    assert m.crc32(1)[0] == A.QZ_OK and m.crc32(2)[0] == A.QZ_OK
    # a byte of record 1 changes behind the library's back.  Where record 1 starts is found, not assumed: a marker written
    # as its offset field is looked for in a second blob of the same shape (the blob is plain host memory)
    probe = A.Metadata(4096, 1024)
    probe.write(1, offset=0x5A5A5A5A)
    rec = C.string_at(probe.h.value, 128).find(b"\x5A\x5A\x5A\x5A")
    probe.free()
    assert rec > 0
    raw = (C.c_ubyte * 1).from_address(m.h.value + rec + 5)       # a byte of block 1's size field
    raw[0] ^= 0x40
    assert m.crc32(1)[0] == A.QZ_PARAMS and m.crc64(1)[0] == A.QZ_PARAMS
    assert m.crc32(0)[0] == A.QZ_OK and m.crc32(2)[0] == A.QZ_OK   # the other records are untouched
    assert m.write(1, size=20) == A.QZ_OK                          # a write refreshes the word
    assert m.crc32(1)[0] == A.QZ_OK
    assert m.free() == A.QZ_OK


def test_smallest_blob_allocates_and_frees(L):
    h = C.c_void_p()
    assert L.qzAllocateMetadata(C.byref(h), 1, 1024) == A.QZ_OK
    assert L.qzFreeMetadata(h) == A.QZ_OK


def test_crc_configs_need_a_session_and_check_their_fields(L):
    s = A.QzSession()
    g64, g32 = A.QzCrc64Config(), A.QzCrc32Config()
    assert L.qzGetSessionCrc64Config(C.byref(s), C.byref(g64)) == A.QZ_FAIL       # never set up
    assert L.qzSetSessionCrc64Config(C.byref(s), C.byref(g64)) == A.QZ_FAIL
    assert L.qzGetSessionCrc32Config(C.byref(s), C.byref(g32)) == A.QZ_FAIL
    assert L.qzSetSessionCrc32Config(C.byref(s), C.byref(g32)) == A.QZ_FAIL
    assert L.qzGetSessionCrc64Config(None, C.byref(g64)) == A.QZ_PARAMS
    S = A.Session(A.QZ_DEFLATE_RAW)                                 # setting a session up needs no device
    assert S.rc_setup == A.QZ_OK
    assert L.qzGetSessionCrc64Config(C.byref(S.s), None) == A.QZ_PARAMS
    assert L.qzSetSessionCrc32Config(C.byref(S.s), None) == A.QZ_PARAMS
    # the defaults: CRC-64/ECMA-182 and the gzip CRC-32
    assert S.get_crc64() == (A.QZ_OK, crcmodel.CRC64_ECMA[1:])
    assert S.get_crc32() == (A.QZ_OK, crcmodel.CRC32_ISO_HDLC[1:])
    assert S.set_crc64(*crcmodel.CRC64_XZ[1:]) == A.QZ_OK and S.get_crc64() == (A.QZ_OK, crcmodel.CRC64_XZ[1:])
    assert S.set_crc32(*crcmodel.CRC32C[1:]) == A.QZ_OK and S.get_crc32() == (A.QZ_OK, crcmodel.CRC32C[1:])
    assert S.set_crc64(0x42F0E1EBA9EA3692, 0, 0, 0, 0) == A.QZ_PARAMS              # bit 0 of the polynomial clear
    assert S.set_crc64(0x1B, 0, 2, 0, 0) == A.QZ_PARAMS and S.set_crc64(0x1B, 0, 0, 7, 0) == A.QZ_PARAMS
    assert S.set_crc32(0x04C11DB6, 0, 0, 0, 0) == A.QZ_PARAMS and S.set_crc32(0x04C11DB7, 0, 1, 2, 0) == A.QZ_PARAMS
    assert S.get_crc64() == (A.QZ_OK, crcmodel.CRC64_XZ[1:]) and S.get_crc32() == (A.QZ_OK, crcmodel.CRC32C[1:])   # a refused config changes nothing
    L.qzTeardownSession(C.byref(S.s))
