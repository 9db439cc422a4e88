"""libzstd through ctypes, where the machine has it: the second reader of every frame the zstd tests produce, and the
yardsticks of tests/golden/gen_zstd.py's ratio records.  The project's rule for liblz4 (refcalls.lz4_pinned) applies: where
the library does not load, the pinned index carries the check, and no GPU test requires it."""
import ctypes as C

_L = None


def lib():
    """libzstd.so.1 or False"""
    global _L
    if _L is None:
        try:
            L = C.CDLL("libzstd.so.1")
            L.ZSTD_decompress.restype = C.c_size_t
            L.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
            L.ZSTD_compress.restype = C.c_size_t
            L.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
            L.ZSTD_compressBound.restype = C.c_size_t
            L.ZSTD_compressBound.argtypes = [C.c_size_t]
            L.ZSTD_isError.argtypes = [C.c_size_t]
            L.ZSTD_getErrorName.restype = C.c_char_p
            L.ZSTD_getErrorName.argtypes = [C.c_size_t]
            L.ZSTD_findFrameCompressedSize.restype = C.c_size_t
            L.ZSTD_findFrameCompressedSize.argtypes = [C.c_char_p, C.c_size_t]
            _L = L
        except OSError:
            _L = False
    return _L


def available():
    return bool(lib())


def version():
    return lib().ZSTD_versionNumber() if lib() else 0


def decompress(stream, cap):
    """ZSTD_decompress of a stream of frames into cap bytes"""
    L = lib()
    dst = C.create_string_buffer(max(cap, 1))
    r = L.ZSTD_decompress(dst, cap, bytes(stream), len(stream))
    if L.ZSTD_isError(r):
        raise ValueError("ZSTD_decompress: " + L.ZSTD_getErrorName(r).decode())
    return dst.raw[:r]


def check(stream, data):
    """where libzstd loads: the stream must decode to data with ZSTD_decompress too"""
    if available():
        got = decompress(stream, len(data))
        assert got == data, "ZSTD_decompress gives other bytes than the strict reader"


def compress(src, level=1):
    L = lib()
    cap = L.ZSTD_compressBound(len(src))
    dst = C.create_string_buffer(cap)
    r = L.ZSTD_compress(dst, cap, bytes(src), len(src), level)
    if L.ZSTD_isError(r):
        raise ValueError("ZSTD_compress: " + L.ZSTD_getErrorName(r).decode())
    return dst.raw[:r]


class _Seq(C.Structure):
    _fields_ = [("offset", C.c_uint), ("litLength", C.c_uint), ("matchLength", C.c_uint), ("rep", C.c_uint)]


def compress_sequences(src, seqs, level=1):
    """ZSTD_compressSequences with explicit block delimiters on (literal length, match length, offset) records - the
    reference's path (utils/qzstd.c:251).  None when this libzstd does not have the call or refuses it."""
    L = lib()
    if not L or not hasattr(L, "ZSTD_compressSequences"):
        return None
    L.ZSTD_createCCtx.restype = C.c_void_p
    L.ZSTD_freeCCtx.argtypes = [C.c_void_p]
    L.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.ZSTD_CCtx_setParameter.restype = C.c_size_t
    L.ZSTD_compressSequences.restype = C.c_size_t
    L.ZSTD_compressSequences.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    cctx = L.ZSTD_createCCtx()
    try:
        # ZSTD_c_compressionLevel 100; ZSTD_c_blockDelimiters (experimental 11) 1008 = ZSTD_sf_explicitBlockDelimiters 1.
        # ZSTD_c_validateSequences stays off, as in the reference: 1.4.8 validates against the LEVEL's minimum match, which
        # refuses the three- and four-byte matches of an LZ4s parse; the callers decode the result instead
        if L.ZSTD_isError(L.ZSTD_CCtx_setParameter(cctx, 100, level)):
            return None
        if L.ZSTD_isError(L.ZSTD_CCtx_setParameter(cctx, 1008, 1)):
            return None
        arr = (_Seq * (len(seqs) + 1))()
        for i, (ll, ml, off) in enumerate(seqs):
            arr[i].offset, arr[i].litLength, arr[i].matchLength = off, ll, ml
        covered = sum(s[0] + s[1] for s in seqs)
        arr[len(seqs)].litLength = len(src) - covered       # the delimiter: offset 0, match length 0, the trailing literals
        cap = L.ZSTD_compressBound(len(src))
        dst = C.create_string_buffer(cap)
        r = L.ZSTD_compressSequences(cctx, dst, cap, arr, len(seqs) + 1, bytes(src), len(src))
        if L.ZSTD_isError(r):
            return None
        return dst.raw[:r]
    finally:
        L.ZSTD_freeCCtx(cctx)
