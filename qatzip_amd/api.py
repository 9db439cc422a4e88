"""ctypes mirror of the qatzip.h application interface exported by libqatzip_amd.so.

Same names, argument meaning and return codes as the reference API (include/qatzip.h), so the parity
tests read like the reference's own tests (test/main.c, test/bt.c)."""
import ctypes as C

from ._lib import load

QZ_OK, QZ_DUPLICATE, QZ_PARAMS, QZ_FAIL, QZ_BUF_ERROR, QZ_DATA_ERROR = 0, 1, -1, -2, -3, -4
QZ_NOT_SUPPORTED, QZ_NOSW_NO_HW, QZ_UNSUPPORTED_FMT = -200, -101, 16
QZ_POST_PROCESS_ERROR = -117
QZ_METADATA_OVERFLOW, QZ_OUT_OF_RANGE = -118, -119
QZ_DEFLATE_4B, QZ_DEFLATE_GZIP, QZ_DEFLATE_GZIP_EXT, QZ_DEFLATE_RAW = 0, 1, 2, 3
QZ_DEFLATE, QZ_LZ4, QZ_LZ4s = 8, ord("4"), ord("s")
QZ_DIR_COMPRESS, QZ_DIR_DECOMPRESS, QZ_DIR_BOTH = 0, 1, 2
COMMON_MEM, PINNED_MEM = 0, 1


class QzSession(C.Structure):
    _fields_ = [("hw_session_stat", C.c_long), ("thd_sess_stat", C.c_int), ("internal", C.c_void_p),
                ("total_in", C.c_ulong), ("total_out", C.c_ulong)]


class QzSessionParams(C.Structure):
    _fields_ = [("huffman_hdr", C.c_int), ("direction", C.c_int), ("data_fmt", C.c_int), ("comp_lvl", C.c_uint),
                ("comp_algorithm", C.c_ubyte), ("max_forks", C.c_uint), ("sw_backup", C.c_ubyte),
                ("hw_buff_sz", C.c_uint), ("strm_buff_sz", C.c_uint), ("input_sz_thrshold", C.c_uint),
                ("req_cnt_thrshold", C.c_uint), ("wait_cnt_thrshold", C.c_uint)]


class QzSessionParamsCommon(C.Structure):
    _fields_ = [("direction", C.c_int), ("comp_lvl", C.c_uint), ("comp_algorithm", C.c_ubyte), ("max_forks", C.c_uint),
                ("sw_backup", C.c_ubyte), ("hw_buff_sz", C.c_uint), ("strm_buff_sz", C.c_uint),
                ("input_sz_thrshold", C.c_uint), ("req_cnt_thrshold", C.c_uint), ("wait_cnt_thrshold", C.c_uint),
                ("polling_mode", C.c_int), ("is_sensitive_mode", C.c_uint)]


class QzSessionParamsDeflate(C.Structure):
    _fields_ = [("common_params", QzSessionParamsCommon), ("huffman_hdr", C.c_int), ("data_fmt", C.c_int)]


class QzSessionParamsDeflateExt(C.Structure):
    _fields_ = [("deflate_params", QzSessionParamsDeflate), ("stop_decompression_stream_end", C.c_ubyte),
                ("zlib_format", C.c_ubyte)]


class QzSessionParamsLZ4(C.Structure):
    _fields_ = [("common_params", QzSessionParamsCommon)]


# qzLZ4SCallbackFn: int cb(void *external, const unsigned char *src, unsigned int *src_len, unsigned char *dest,
#                          unsigned int *dest_len, int *ExtStatus)
QzLZ4SCallback = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint), C.c_void_p, C.POINTER(C.c_uint),
                             C.POINTER(C.c_int))


class QzSessionParamsLZ4S(C.Structure):
    _fields_ = [("common_params", QzSessionParamsCommon), ("qzCallback", QzLZ4SCallback), ("qzCallback_external", C.c_void_p),
                ("lz4s_mini_match", C.c_uint)]


class QzStream(C.Structure):
    _fields_ = [("in_sz", C.c_uint), ("out_sz", C.c_uint), ("in_", C.c_void_p), ("out", C.c_void_p),
                ("pending_in", C.c_uint), ("pending_out", C.c_uint), ("crc_type", C.c_int), ("crc_32", C.c_uint),
                ("reserved", C.c_ulonglong), ("opaque", C.c_void_p)]


class QzResult(C.Structure):
    _fields_ = [("status", C.c_int), ("cb_tag", C.c_void_p), ("src_len", C.c_uint), ("dest_len", C.c_uint),
                ("ext_rc", C.c_uint64), ("crc", C.c_void_p), ("extension_result", C.c_void_p)]


class QzCrc64Config(C.Structure):
    _fields_ = [("polynomial", C.c_uint64), ("initial_value", C.c_uint64), ("reflect_in", C.c_uint32),
                ("reflect_out", C.c_uint32), ("xor_out", C.c_uint64)]


class QzCrc32Config(C.Structure):
    _fields_ = [("polynomial", C.c_uint32), ("initial_value", C.c_uint32), ("reflect_in", C.c_uint32),
                ("reflect_out", C.c_uint32), ("xor_out", C.c_uint32)]


QzAsyncCallback = C.CFUNCTYPE(C.c_int, C.POINTER(QzResult))

_bound = False


def lib():
    global _bound
    L = load()
    if not _bound:
        P, u8p, up = C.POINTER, C.c_char_p, C.POINTER(C.c_uint)
        L.qzInit.argtypes = [P(QzSession), C.c_ubyte]
        L.qzSetupSession.argtypes = [P(QzSession), P(QzSessionParams)]
        L.qzSetupSessionDeflate.argtypes = [P(QzSession), P(QzSessionParamsDeflate)]
        L.qzSetupSessionLZ4.argtypes = [P(QzSession), P(QzSessionParamsLZ4)]
        L.qzGetDefaults.argtypes = [P(QzSessionParams)]
        L.qzSetDefaults.argtypes = [P(QzSessionParams)]
        L.qzGetDefaultsDeflate.argtypes = [P(QzSessionParamsDeflate)]
        L.qzGetDefaultsLZ4.argtypes = [P(QzSessionParamsLZ4)]
        L.qzSetupSessionLZ4S.argtypes = [P(QzSession), P(QzSessionParamsLZ4S)]
        L.qzSetupSessionZstdAMD.argtypes = [P(QzSession), P(QzSessionParamsLZ4S)]
        L.qzSetupSessionZstdDecAMD.argtypes = [P(QzSession), P(QzSessionParamsLZ4S)]
        L.qzGetDefaultsLZ4S.argtypes = [P(QzSessionParamsLZ4S)]
        L.qzSetDefaultsLZ4S.argtypes = [P(QzSessionParamsLZ4S)]
        L.qzCompressExt.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, C.c_uint, P(C.c_uint64)]
        L.qzCompressCrcExt.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, C.c_uint, P(C.c_ulong), P(C.c_uint64)]
        L.qzGetDefaultsDeflateExt.argtypes = [P(QzSessionParamsDeflateExt)]
        L.qzSetupSessionDeflateExt.argtypes = [P(QzSession), P(QzSessionParamsDeflateExt)]
        L.qzCompress.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, C.c_uint]
        L.qzCompressCrc.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, C.c_uint, P(C.c_ulong)]
        L.qzDecompress.argtypes = [P(QzSession), u8p, up, C.c_void_p, up]
        L.qzDecompressCrc.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, P(C.c_ulong)]
        L.qzTeardownSession.argtypes = [P(QzSession)]
        L.qzClose.argtypes = [P(QzSession)]
        L.qzMaxCompressedLength.argtypes = [C.c_uint, P(QzSession)]
        L.qzMaxCompressedLength.restype = C.c_uint
        L.qzMalloc.argtypes = [C.c_size_t, C.c_int, C.c_int]; L.qzMalloc.restype = C.c_void_p
        L.qzFree.argtypes = [C.c_void_p]; L.qzFree.restype = None
        L.qzMemFindAddr.argtypes = [C.c_void_p]
        L.qzCompressStream.argtypes = [P(QzSession), P(QzStream), C.c_uint]
        L.qzDecompressStream.argtypes = [P(QzSession), P(QzStream), C.c_uint]
        L.qzEndStream.argtypes = [P(QzSession), P(QzStream)]
        L.qzSetLogLevel.argtypes = [C.c_int]
        L.qzCompress2.argtypes = [P(QzSession), C.c_void_p, C.c_void_p, C.c_void_p, P(QzResult)]
        L.qzDecompress2.argtypes = [P(QzSession), C.c_void_p, C.c_void_p, C.c_void_p, P(QzResult)]
        u32p, u64p = P(C.c_uint32), P(C.c_uint64)
        L.qzCompressCrc64.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, C.c_uint, u64p]
        L.qzCompressCrc64Ext.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, C.c_uint, u64p, u64p]
        L.qzDecompressCrc64.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, u64p]
        L.qzDecompressCrc64Ext.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, u64p, u64p]
        L.qzCompressWithMetadataExt.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, C.c_uint, u64p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.qzDecompressWithMetadataExt.argtypes = [P(QzSession), u8p, up, C.c_void_p, up, u64p, C.c_void_p, C.c_uint32]
        L.qzAllocateMetadata.argtypes = [P(C.c_void_p), C.c_size_t, C.c_uint32]
        L.qzFreeMetadata.argtypes = [C.c_void_p]
        L.qzMetadataBlockRead.argtypes = [C.c_uint32, C.c_void_p, u32p, u32p, u32p, u32p]
        L.qzMetadataBlockWrite.argtypes = [C.c_uint32, C.c_void_p, u32p, u32p, u32p, u32p]
        L.qzMetadataBlockGetCrc64.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p]
        L.qzMetadataBlockGetCrc32.argtypes = [C.c_uint32, C.c_void_p, u32p, u32p]
        L.qzGetSessionCrc64Config.argtypes = [P(QzSession), P(QzCrc64Config)]
        L.qzSetSessionCrc64Config.argtypes = [P(QzSession), P(QzCrc64Config)]
        L.qzGetSessionCrc32Config.argtypes = [P(QzSession), P(QzCrc32Config)]
        L.qzSetSessionCrc32Config.argtypes = [P(QzSession), P(QzCrc32Config)]
        L.qzSetSessionZstdSeqAMD.argtypes = [P(QzSession), C.c_uint]
        L.qzSetSessionZstdParseAMD.argtypes = [P(QzSession), C.c_uint]
        if hasattr(L, "qzSetSessionZstdDecodeRouteAMD"):
            L.qzSetSessionZstdDecodeRouteAMD.argtypes = [P(QzSession), C.c_int]
        _bound = True
    return L


class Metadata:
    """A QzMetadataBlob_T (qzAllocateMetadata): one record per hw_buff_sz block of data_size bytes."""

    def __init__(self, data_size, hw_buff_sz):
        self.L = lib()
        self.h = C.c_void_p()
        self.rc_alloc = self.L.qzAllocateMetadata(C.byref(self.h), data_size, hw_buff_sz)

    def read(self, k):
        """-> (rc, offset, size, flags, hash)"""
        o, z, f, h = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = self.L.qzMetadataBlockRead(k, self.h, C.byref(o), C.byref(z), C.byref(f), C.byref(h))
        return rc, o.value, z.value, f.value, h.value

    def write(self, k, offset=None, size=None, flags=None, hash=None):
        """qzMetadataBlockWrite; a field left None is passed as NULL (not written)"""
        a = [None if v is None else C.byref(C.c_uint32(v)) for v in (offset, size, flags, hash)]
        return self.L.qzMetadataBlockWrite(k, self.h, *a)

    def crc32(self, k):
        """-> (rc, input_crc, output_crc)"""
        i, o = C.c_uint32(), C.c_uint32()
        rc = self.L.qzMetadataBlockGetCrc32(k, self.h, C.byref(i), C.byref(o))
        return rc, i.value, o.value

    def crc64(self, k):
        i, o = C.c_uint64(), C.c_uint64()
        rc = self.L.qzMetadataBlockGetCrc64(k, self.h, C.byref(i), C.byref(o))
        return rc, i.value, o.value

    def free(self):
        rc = self.L.qzFreeMetadata(self.h) if self.h else QZ_PARAMS
        self.h = C.c_void_p()
        return rc


QZ_ZSTD_SEQ_FSE_TABLES, QZ_ZSTD_SEQ_REPEAT_OFFSETS = 1, 2      # include/qzamd_zstd_seq.h


class Session:
    """A QzSession_T set up the way test/main.c does it: qzGetDefaults -> tweak -> qzSetupSession."""

    def __init__(self, data_fmt=QZ_DEFLATE_GZIP_EXT, hw_buff_sz=65536, comp_lvl=1, lz4=False, strm_buff_sz=None,
                 zlib_format=False, stop_at_stream_end=False, lz4s=False, mini_match=3, callback=None, external=None,
                 zstd=False, zstd_dec=None):
        self.L = lib()
        self.s = QzSession()
        self.cb = None
        if lz4s or zstd or zstd_dec is not None:
            # an LZ4s session (qzSetupSessionLZ4S): compress only; callback is a Python callable with qzLZ4SCallbackFn's
            # arguments (or a QzLZ4SCallback), kept alive by this object for as long as the session may call it
            p = QzSessionParamsLZ4S(); self.L.qzGetDefaultsLZ4S(C.byref(p))
            p.common_params.comp_algorithm = QZ_LZ4s; p.common_params.direction = QZ_DIR_COMPRESS
            p.common_params.hw_buff_sz = hw_buff_sz; p.common_params.comp_lvl = comp_lvl
            p.lz4s_mini_match = mini_match
            if callback is not None:
                self.cb = callback if isinstance(callback, QzLZ4SCallback) else QzLZ4SCallback(callback)
                p.qzCallback = self.cb
            p.qzCallback_external = external
            # zstd: a zstd session (qzSetupSessionZstdAMD, include/qzamd_zstd.h) - the same parameters, a zstd frame per chunk
            setup = self.L.qzSetupSessionZstdAMD if zstd else self.L.qzSetupSessionLZ4S
            # zstd_dec: a zstd decode session (qzSetupSessionZstdDecAMD, include/qzamd_zstd_dec.h) with that direction
            if zstd_dec is not None:
                p.common_params.direction = zstd_dec
                setup = self.L.qzSetupSessionZstdDecAMD
            self.rc_setup = setup(C.byref(self.s), C.byref(p))
        elif zlib_format or stop_at_stream_end:  # qzSetupSessionDeflateExt: zlib_format = 1 is the RFC 1950 wrapper with an Adler-32 trailer
            p = QzSessionParamsDeflateExt(); self.L.qzGetDefaultsDeflateExt(C.byref(p))
            if zlib_format:
                p.deflate_params.data_fmt = QZ_DEFLATE_RAW; p.zlib_format = 1
            else:
                p.deflate_params.data_fmt = data_fmt
            p.stop_decompression_stream_end = 1 if stop_at_stream_end else 0
            p.deflate_params.common_params.hw_buff_sz = hw_buff_sz; p.deflate_params.common_params.comp_lvl = comp_lvl
            self.rc_setup = self.L.qzSetupSessionDeflateExt(C.byref(self.s), C.byref(p))
        elif lz4:
            p = QzSessionParamsLZ4(); self.L.qzGetDefaultsLZ4(C.byref(p))
            p.common_params.comp_algorithm = QZ_LZ4
            p.common_params.hw_buff_sz = hw_buff_sz; p.common_params.comp_lvl = comp_lvl
            self.rc_setup = self.L.qzSetupSessionLZ4(C.byref(self.s), C.byref(p))
        else:
            p = QzSessionParams(); self.L.qzGetDefaults(C.byref(p))
            p.data_fmt = data_fmt; p.hw_buff_sz = hw_buff_sz; p.comp_lvl = comp_lvl
            if strm_buff_sz:
                p.strm_buff_sz = strm_buff_sz
            self.rc_setup = self.L.qzSetupSession(C.byref(self.s), C.byref(p))

    def compress(self, src: bytes, last=1, cap=None, crc0=None):
        """-> (rc, consumed, out_bytes, crc)"""
        if cap is None:
            cap = self.L.qzMaxCompressedLength(max(len(src), 1), C.byref(self.s)) + 64
        sl, dl = C.c_uint(len(src)), C.c_uint(cap)
        dst = C.create_string_buffer(max(cap, 1))
        if crc0 is None:
            rc = self.L.qzCompress(C.byref(self.s), src, C.byref(sl), dst, C.byref(dl), last)
            return rc, sl.value, dst.raw[:dl.value], None
        crc = C.c_ulong(crc0)
        rc = self.L.qzCompressCrc(C.byref(self.s), src, C.byref(sl), dst, C.byref(dl), last, C.byref(crc))
        return rc, sl.value, dst.raw[:dl.value], crc.value

    def compress_ext(self, src, last=1, cap=None):
        """qzCompressExt -> (rc, consumed, out_bytes, ext_rc); src: bytes or a ctypes buffer (whose address the callback of an
        LZ4s session then sees)"""
        n = len(src)
        if cap is None:
            cap = self.L.qzMaxCompressedLength(max(n, 1), C.byref(self.s)) + 64
        sl, dl, ext = C.c_uint(n), C.c_uint(cap), C.c_uint64(7)
        dst = C.create_string_buffer(max(cap, 1))
        a = src if isinstance(src, bytes) else C.cast(src, C.c_char_p)
        rc = self.L.qzCompressExt(C.byref(self.s), a, C.byref(sl), dst, C.byref(dl), last, C.byref(ext))
        return rc, sl.value, dst.raw[:dl.value], ext.value

    def decompress(self, comp: bytes, cap: int, crc0=0, want_crc=False):
        """-> (rc, consumed, out_bytes[, crc]): qzDecompress, or qzDecompressCrc (running CRC-32 of the output) with want_crc"""
        sl, dl = C.c_uint(len(comp)), C.c_uint(cap)
        dst = C.create_string_buffer(max(cap, 1))
        if want_crc:
            crc = C.c_ulong(crc0)
            rc = self.L.qzDecompressCrc(C.byref(self.s), comp, C.byref(sl), dst, C.byref(dl), C.byref(crc))
            return rc, sl.value, dst.raw[:dl.value], crc.value
        rc = self.L.qzDecompress(C.byref(self.s), comp, C.byref(sl), dst, C.byref(dl))
        return rc, sl.value, dst.raw[:dl.value]

    def compress_crc64(self, src: bytes, crc0=0, last=1, cap=None):
        """qzCompressCrc64 -> (rc, consumed, out_bytes, crc): crc0 = the finalised CRC-64 of the bytes before this call"""
        if cap is None:
            cap = self.L.qzMaxCompressedLength(max(len(src), 1), C.byref(self.s)) + 64
        sl, dl, crc = C.c_uint(len(src)), C.c_uint(cap), C.c_uint64(crc0)
        dst = C.create_string_buffer(max(cap, 1))
        rc = self.L.qzCompressCrc64(C.byref(self.s), src, C.byref(sl), dst, C.byref(dl), last, C.byref(crc))
        return rc, sl.value, dst.raw[:dl.value], crc.value

    def decompress_crc64(self, comp: bytes, cap: int, crc0=0):
        """qzDecompressCrc64 -> (rc, consumed, out_bytes, crc of the output)"""
        sl, dl, crc = C.c_uint(len(comp)), C.c_uint(cap), C.c_uint64(crc0)
        dst = C.create_string_buffer(max(cap, 1))
        rc = self.L.qzDecompressCrc64(C.byref(self.s), comp, C.byref(sl), dst, C.byref(dl), C.byref(crc))
        return rc, sl.value, dst.raw[:dl.value], crc.value

    def set_crc64(self, polynomial, initial_value, reflect_in, reflect_out, xor_out):
        g = QzCrc64Config(polynomial, initial_value, reflect_in, reflect_out, xor_out)
        return self.L.qzSetSessionCrc64Config(C.byref(self.s), C.byref(g))

    def set_zstd_seq(self, flags):
        """qzSetSessionZstdSeqAMD (include/qzamd_zstd_seq.h): QZ_ZSTD_SEQ_FSE_TABLES | QZ_ZSTD_SEQ_REPEAT_OFFSETS, 0 for neither"""
        return self.L.qzSetSessionZstdSeqAMD(C.byref(self.s), flags)

    def set_zstd_parse(self, depth):
        """qzSetSessionZstdParseAMD (include/qzamd_zstd_parse.h): 0 the default parse, 1 .. 256 the search attempts per position
        of the hash-chain lazy parse"""
        return self.L.qzSetSessionZstdParseAMD(C.byref(self.s), depth)

    ZSTDD_ROUTES = {"auto": 0, "frame": 1, "blocks": 2}

    def zstd_decode_route(self, route):
        """qzSetSessionZstdDecodeRouteAMD (include/qzamd_zstd_blocks.h): "auto", "frame" or "blocks" for the qzDecompress calls of
        a zstd decode session from now on"""
        return self.L.qzSetSessionZstdDecodeRouteAMD(C.byref(self.s), self.ZSTDD_ROUTES.get(route, route))

    def set_crc32(self, polynomial, initial_value, reflect_in, reflect_out, xor_out):
        g = QzCrc32Config(polynomial, initial_value, reflect_in, reflect_out, xor_out)
        return self.L.qzSetSessionCrc32Config(C.byref(self.s), C.byref(g))

    def get_crc64(self):
        g = QzCrc64Config()
        rc = self.L.qzGetSessionCrc64Config(C.byref(self.s), C.byref(g))
        return rc, (g.polynomial, g.initial_value, g.reflect_in, g.reflect_out, g.xor_out)

    def get_crc32(self):
        g = QzCrc32Config()
        rc = self.L.qzGetSessionCrc32Config(C.byref(self.s), C.byref(g))
        return rc, (g.polynomial, g.initial_value, g.reflect_in, g.reflect_out, g.xor_out)

    def compress_meta(self, src: bytes, meta, thrshold, override=0, cap=None, last=1):
        """qzCompressWithMetadataExt -> (rc, consumed, out_bytes); last_ext_rc <- what the call left in *ext_rc"""
        if cap is None:
            cap = len(src) + len(src) // 8 + 1024
        sl, dl = C.c_uint(len(src)), C.c_uint(cap)
        dst = C.create_string_buffer(max(cap, 1))
        ext = C.c_uint64(7)
        rc = self.L.qzCompressWithMetadataExt(C.byref(self.s), src, C.byref(sl), dst, C.byref(dl), last, C.byref(ext), meta.h,
                                              override, thrshold)
        self.last_ext_rc = ext.value
        return rc, sl.value, dst.raw[:dl.value]

    def decompress_meta(self, comp: bytes, meta, cap, override=0):
        """qzDecompressWithMetadataExt -> (rc, consumed, out_bytes)"""
        sl, dl = C.c_uint(len(comp)), C.c_uint(cap)
        dst = C.create_string_buffer(max(cap, 1))
        rc = self.L.qzDecompressWithMetadataExt(C.byref(self.s), comp, C.byref(sl), dst, C.byref(dl), None, meta.h, override)
        return rc, sl.value, dst.raw[:dl.value]

    def end_of_stream(self):
        """qzGetDeflateEndOfStream: 1 if the last decompress call ended on the end of a deflate stream"""
        e = C.c_ubyte(7)
        rc = self.L.qzGetDeflateEndOfStream(C.byref(self.s), C.byref(e))
        return rc, e.value

    def close(self):
        self.L.qzTeardownSession(C.byref(self.s))
        self.L.qzClose(C.byref(self.s))
