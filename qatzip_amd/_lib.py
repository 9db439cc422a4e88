"""ctypes view of libqatzip_amd.so's device-resident C ABI (include/qzamd_device.h).

There is deliberately no fallback: if the HIP library is missing or no GPU is present
the constructors raise.  (The CPU oracle lives under oracle/ and is test-only.)
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_lib = None


class QzdError(RuntimeError):
    pass


class CrcCfg(C.Structure):
    """qzd_crccfg: a CRC in the Rocksoft model (width 32: the 64-bit fields hold 32-bit values)"""
    _fields_ = [("polynomial", C.c_uint64), ("initial_value", C.c_uint64), ("reflect_in", C.c_uint32),
                ("reflect_out", C.c_uint32), ("xor_out", C.c_uint64)]


def load(build_if_missing=True):
    global _lib
    if _lib is not None:
        return _lib
    so = os.environ.get("QATZIP_AMD_SO") or _build.SO      # developer switch: a variant build of the same library
    if not os.path.exists(so):
        if not build_if_missing:
            raise QzdError("libqatzip_amd.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`)")
        _build.build()
    L = C.CDLL(so)
    vp, u8p = C.c_void_p, C.c_void_p
    L.qzd_device_count.restype = C.c_int
    L.qzd_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.qzd_destroy.argtypes = [vp]
    L.qzd_last_error.argtypes = [vp]; L.qzd_last_error.restype = C.c_char_p
    L.qzd_batch_chunks.argtypes = [vp]; L.qzd_batch_chunks.restype = C.c_uint32
    L.qzd_k1_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]
    L.qzd_inflate_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]
    L.qzd_stream_copy_peak.argtypes = [vp, C.c_uint64, C.c_int, C.POINTER(C.c_double)]
    L.qzd_dev_alloc.argtypes = [vp, C.c_size_t]; L.qzd_dev_alloc.restype = vp
    L.qzd_dev_free.argtypes = [vp, vp]
    L.qzd_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.qzd_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    L.qzd_deflate_raw.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, u8p, C.c_uint64,
                                  C.POINTER(C.c_uint64), vp]
    L.qzd_deflate_raw_async.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, u8p, C.c_uint64]
    L.qzd_sync.argtypes = [vp]
    L.qzd_result.argtypes = [vp, C.POINTER(C.c_uint64), vp, C.c_uint32]
    L.qzd_last_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    L.qzd_inflate_segments.argtypes = [vp, u8p, u8p, vp, C.c_uint32, vp]
    L.qzd_inflate_stream.argtypes = [vp, u8p, C.c_uint64, u8p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.qzd_crc32.argtypes = [vp, u8p, C.c_uint64, C.POINTER(C.c_uint32)]
    L.qzd_crc32_ranges.argtypes = [vp, u8p, vp, C.c_uint32, vp]
    L.qzd_last_inflate_timing.argtypes = [vp, C.POINTER(C.c_float * 4)]
    if hasattr(L, "qzd_inflate_scratch_bytes"):            # (variant libraries built from older sources lack it; the export test does not)
        L.qzd_inflate_scratch_bytes.argtypes = [vp]; L.qzd_inflate_scratch_bytes.restype = C.c_uint64
    L.qzd_d2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.qzd_lz4_compress_frames.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, u8p, C.c_uint64, C.POINTER(C.c_uint64), vp]
    L.qzd_lz4_compress_frames_hw.argtypes = L.qzd_lz4_compress_frames.argtypes
    L.qzd_lz4_compress_linked.argtypes = [vp, u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.qzd_lz4_decompress_frames.argtypes = [vp, u8p, u8p, vp, C.c_uint32, vp]
    if hasattr(L, "qzd_lz4_decode_route"):                  # (variant libraries built from older sources lack it)
        L.qzd_lz4_decode_route.argtypes = [vp, C.c_int]
    L.qzd_lz4hc_compress_frames.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, C.c_int, u8p, C.c_uint64, C.POINTER(C.c_uint64), vp]
    L.qzd_lz4hc_compress_frames_hw.argtypes = L.qzd_lz4hc_compress_frames.argtypes
    L.qzd_lz4hc_compress_linked.argtypes = [vp, u8p, C.c_uint64, C.c_int, u8p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.qzd_lz4s_bound.argtypes = [C.c_uint64, C.c_uint32]; L.qzd_lz4s_bound.restype = C.c_uint64
    L.qzd_lz4s_compress_blocks.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, u8p, C.c_uint64,
                                           C.POINTER(C.c_uint64), vp]
    L.qzd_zstd_bound.argtypes = [C.c_uint64, C.c_uint32]; L.qzd_zstd_bound.restype = C.c_uint64
    L.qzd_zstd_compress_frames.argtypes = L.qzd_lz4s_compress_blocks.argtypes
    L.qzd_zstd_encode_frames.argtypes = [vp, u8p, vp, vp, C.c_uint32, u8p, C.c_uint64, C.POINTER(C.c_uint64), vp]
    L.qzd_zstd_compress_frames_ex.argtypes = L.qzd_zstd_compress_frames.argtypes + [C.c_uint32]
    L.qzd_zstd_encode_frames_ex.argtypes = L.qzd_zstd_encode_frames.argtypes + [C.c_uint32]
    L.qzd_zstd_compress_frames_parse.argtypes = L.qzd_zstd_compress_frames.argtypes + [C.c_uint32, C.c_uint32]
    L.qzd_zstd_decompress_frames.argtypes = [vp, u8p, u8p, vp, C.c_uint32, vp]
    if hasattr(L, "qzd_zstd_decompress_frames_ex"):         # (variant libraries built from older sources lack them)
        L.qzd_zstd_decompress_frames_ex.argtypes = [vp, u8p, u8p, vp, C.c_uint32, vp, vp]
        L.qzd_zstd_count_blocks.argtypes = [vp, u8p, vp, C.c_uint32, vp]
        L.qzd_zstd_decode_route.argtypes = [vp, C.c_int]
    L.qzd_chunk_lens.argtypes = [vp, vp, C.c_uint32]
    L.qzd_shard_root_create.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_char_p, C.POINTER(vp)]
    L.qzd_shard_attach.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(vp)]
    L.qzd_shard_slot_handle.argtypes = [vp, C.c_uint32, C.c_char_p]
    L.qzd_shard_attach_slot.argtypes = [vp, C.c_char_p]
    L.qzd_shard_put.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.POINTER(C.c_uint64)]
    L.qzd_shard_finish.argtypes = [vp, C.c_uint32, C.c_double, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint64)]
    L.qzd_shard_close.argtypes = [vp]
    L.qzd_rccl_unique_id.argtypes = [C.c_char_p]
    L.qzd_rccl_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(vp)]
    L.qzd_rccl_gather.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.qzd_rccl_close.argtypes = [vp]
    L.qzd_ctx_device.argtypes = [vp]
    L.qzd_pcie_peak.argtypes = [vp, C.c_uint64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.qzd_crc32_fold.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64]; L.qzd_crc32_fold.restype = C.c_uint32
    L.qzd_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]; L.qzd_crc32_combine.restype = C.c_uint32
    L.qzd_crcn_ranges.argtypes = [vp, u8p, vp, C.c_uint32, C.c_int, C.POINTER(CrcCfg), vp, vp]
    L.qzd_xxh32_ranges.argtypes = [vp, u8p, vp, C.c_uint32, vp]
    L.qzd_blocks_compress.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(CrcCfg), C.POINTER(CrcCfg),
                                      u8p, C.c_uint64, vp, C.POINTER(C.c_uint64)]
    L.qzd_blocks_decompress.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint32, u8p, C.c_uint64, vp, C.POINTER(C.c_uint64)]
    _lib = L
    return L


SEG_DT = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("in_len", "<u4"), ("out_cap", "<u4"),
                   ("flags", "<u4"), ("pad", "<u4")])
RES_DT = np.dtype([("status", "<i4"), ("in_used", "<u4"), ("out_len", "<u4"), ("nblocks", "<u4")])
LZ4SEG_DT = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("in_len", "<u4"), ("out_cap", "<u4")])
LZ4RES_DT = np.dtype([("status", "<i4"), ("in_used", "<u4"), ("out_len", "<u4"), ("pad", "<u4")])
RANGE_DT = np.dtype([("off", "<u8"), ("len", "<u4"), ("pad", "<u4")])
BLOCKREC_DT = np.dtype([("offset", "<u8"), ("size", "<u4"), ("flags", "<u4"), ("hash", "<u4"), ("in_crc32", "<u4"),
                        ("out_crc32", "<u4"), ("pad", "<u4"), ("in_crc64", "<u8"), ("out_crc64", "<u8")])


def exported_symbols():
    """Names include/*.h declares that must be exported by the library (checked on CPU too)."""
    return ["qzd_create", "qzd_destroy", "qzd_last_error", "qzd_device_count", "qzd_ctx_device", "qzd_dev_alloc", "qzd_dev_free",
            "qzd_h2d", "qzd_d2h", "qzd_host_alloc_pinned", "qzd_host_free_pinned", "qzd_deflate_raw",
            "qzd_deflate_raw_async", "qzd_sync", "qzd_result", "qzd_last_timing", "qzd_inflate_segments",
            "qzd_inflate_stream", "qzd_crc32", "qzd_crc32_ranges", "qzd_last_inflate_timing", "qzd_inflate_scratch_bytes",
            "qzd_lz4_compress_frames", "qzd_lz4_compress_frames_hw", "qzd_lz4_decompress_frames", "qzd_lz4_decode_route", "qzd_chunk_lens", "qzd_batch_chunks", "qzd_k1_stats", "qzd_inflate_stats",
            "qzd_adler32_chunks", "qzd_adler32_combine", "qzd_stream_copy_peak", "qzd_deflate_raw_from_host",
            "qzd_deflate_slots", "qzd_inflate_stream_to_host", "qzd_inflate_stream_from_host", "qzamd_async_stats", "qzd_shard_root_create",
            "qzd_shard_attach", "qzd_shard_slot_handle", "qzd_shard_attach_slot", "qzd_lz4_compress_linked", "qzd_shard_put", "qzd_shard_finish", "qzd_shard_close", "qzd_crc32_combine",
            "qzd_lz4hc_compress_frames", "qzd_lz4hc_compress_frames_hw", "qzd_lz4hc_compress_linked",
            "qzd_lz4s_bound", "qzd_lz4s_compress_blocks",
            "qzd_zstd_bound", "qzd_zstd_compress_frames", "qzd_zstd_encode_frames", "qzd_zstd_decompress_frames",
            "qzd_zstd_decompress_frames_ex", "qzd_zstd_count_blocks", "qzd_zstd_decode_route",
            "qzd_zstd_compress_frames_ex", "qzd_zstd_encode_frames_ex", "qzd_zstd_compress_frames_parse",
            "qzd_crcn_ranges", "qzd_xxh32_ranges", "qzd_blocks_compress", "qzd_blocks_decompress",
            "qzd_crc32_fold", "qzd_pcie_peak", "qzd_rccl_unique_id", "qzd_rccl_create", "qzd_rccl_gather", "qzd_rccl_close"]


class DevBuf:
    """A plain HBM allocation owned by a Context."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        self.ptr = ctx.L.qzd_dev_alloc(ctx.h, self.nbytes + 512)   # slack: kernels may look a few bytes ahead
        if not self.ptr:
            raise QzdError("hipMalloc failed for %d bytes" % nbytes)

    def upload(self, data, offset=0):
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1)
        assert offset + a.size <= self.nbytes
        if a.size:
            a = np.ascontiguousarray(a)
            self.ctx._chk(self.ctx.L.qzd_h2d(self.ctx.h, self.ptr + offset, a.ctypes.data, a.size))

    def download(self, n=None, offset=0):
        n = self.nbytes - offset if n is None else int(n)
        out = np.empty(n, np.uint8)
        if n:
            self.ctx._chk(self.ctx.L.qzd_d2h(self.ctx.h, out.ctypes.data, self.ptr + offset, n))
        return out

    def free(self):
        if self.ptr:
            self.ctx.L.qzd_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """qzd_ctx wrapper: one per (process, GPU)."""

    def __init__(self, device=0):
        self.L = load()
        if self.L.qzd_device_count() <= 0:
            raise QzdError("no HIP device visible: the MI355X backend has no CPU fallback")
        h = C.c_void_p()
        rc = self.L.qzd_create(device, C.byref(h))
        if rc != 0:
            raise QzdError("qzd_create failed rc=%d" % rc)
        self.h = h
        self.device = device

    def _chk(self, rc):
        if rc != 0:
            raise QzdError("rc=%d: %s" % (rc, self.L.qzd_last_error(self.h).decode()))

    def alloc(self, n):
        return DevBuf(self, n)

    def close(self):
        if self.h:
            self.L.qzd_destroy(self.h)
            self.h = None

    # -- deflate
    def deflate_raw(self, d_src, n, chunk_sz=65536, level=1, last=1, d_dst=None, want_crc=True):
        """-> (out_len, crc array or None)"""
        nchunks = max(1, (n + chunk_sz - 1) // chunk_sz)
        out_len = C.c_uint64(0)
        crcs = np.zeros(nchunks, np.uint32) if want_crc else None
        self._chk(self.L.qzd_deflate_raw(self.h, d_src.ptr, n, chunk_sz, level, last, d_dst.ptr, d_dst.nbytes,
                                         C.byref(out_len), crcs.ctypes.data if want_crc else None))
        return out_len.value, crcs

    def deflate_raw_async(self, d_src, n, chunk_sz, level, last, d_dst):
        self._chk(self.L.qzd_deflate_raw_async(self.h, d_src.ptr, n, chunk_sz, level, last, d_dst.ptr, d_dst.nbytes))

    def sync(self):
        self._chk(self.L.qzd_sync(self.h))

    def result(self):
        out_len = C.c_uint64(0)
        self._chk(self.L.qzd_result(self.h, C.byref(out_len), None, 0))
        return out_len.value

    def stream_copy_peak(self, nbytes=1 << 30, iters=3):
        """measured HBM stream-copy rate, GB/s of read + written bytes"""
        g = C.c_double(0)
        self._chk(self.L.qzd_stream_copy_peak(self.h, nbytes, iters, C.byref(g)))
        return g.value

    def pcie_peak(self, nbytes=1 << 30, iters=2):
        """pinned hipMemcpyAsync rates (host -> device, device -> host), GB/s"""
        a, b = C.c_double(0), C.c_double(0)
        self._chk(self.L.qzd_pcie_peak(self.h, nbytes, iters, C.byref(a), C.byref(b)))
        return a.value, b.value

    def batch_chunks(self):
        return int(self.L.qzd_batch_chunks(self.h))

    def k1_stats(self, reset=False):
        """(total ms, launches, chunks) of the LZ77 kernel since the last reset"""
        ms, ln, ch = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        self.L.qzd_k1_stats(self.h, C.byref(ms), C.byref(ln), C.byref(ch), 1 if reset else 0)
        return ms.value, ln.value, ch.value

    def inflate_stats(self, reset=False):
        """(segments the K-lane phase A handed back, decode steps re-run with one lane a segment) since the last reset"""
        hb, rr = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.L.qzd_inflate_stats(self.h, C.byref(hb), C.byref(rr), 1 if reset else 0))
        return hb.value, rr.value

    def timing(self):
        ms = (C.c_float * 4)()
        self.L.qzd_last_timing(self.h, C.byref(ms))
        return list(ms)

    # -- inflate
    def inflate_segments(self, d_comp, d_out, segs):
        """segs: list of (in_off, out_off, in_len, out_cap, flags[, pad]) -> structured result array.  pad, when given, is
        the segment's compressed length: with it on every segment the K-lanes-per-segment phase A may take them"""
        sa = np.array([tuple(s) + (0,) * (6 - len(s)) for s in segs], dtype=SEG_DT)
        res = np.zeros(len(segs), RES_DT)
        self._chk(self.L.qzd_inflate_segments(self.h, d_comp.ptr, d_out.ptr, sa.ctypes.data, len(segs), res.ctypes.data))
        return res

    def inflate_stream(self, d_src, n, d_dst, seg_hint=65536, want_crc=True, src_off=0):
        """-> (in_used, out_len, crc or None); raises QzdError on corrupt data / short destination"""
        iu, ol, crc = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        self._chk(self.L.qzd_inflate_stream(self.h, d_src.ptr + src_off, n, d_dst.ptr, d_dst.nbytes, seg_hint,
                                            C.byref(iu), C.byref(ol), C.byref(crc) if want_crc else None))
        return iu.value, ol.value, (crc.value if want_crc else None)

    def crc32(self, d_data, n):
        crc = C.c_uint32(0)
        self._chk(self.L.qzd_crc32(self.h, d_data.ptr, n, C.byref(crc)))
        return crc.value

    # -- block-addressable compression
    def crcn_ranges(self, d_data, ranges, width, cfg, start=None):
        """ranges: list of (off, len); cfg: (polynomial, initial_value, reflect_in, reflect_out, xor_out); start: per range the
        finalised CRC of the bytes before it -> array of finalised CRCs"""
        ra = np.array([(o, n, 0) for o, n in ranges], dtype=RANGE_DT)
        out = np.zeros(len(ranges), np.uint64)
        st = None if start is None else np.array(start, np.uint64)
        self._chk(self.L.qzd_crcn_ranges(self.h, d_data.ptr, ra.ctypes.data, len(ranges), width, C.byref(CrcCfg(*cfg)),
                                         None if st is None else st.ctypes.data, out.ctypes.data))
        return out

    def xxh32_ranges(self, d_data, ranges):
        ra = np.array([(o, n, 0) for o, n in ranges], dtype=RANGE_DT)
        out = np.zeros(len(ranges), np.uint32)
        self._chk(self.L.qzd_xxh32_ranges(self.h, d_data.ptr, ra.ctypes.data, len(ranges), out.ctypes.data))
        return out

    def blocks_compress(self, d_src, n, block_sz, level, thrshold, d_dst, dst_cap=None, cfg32=None, cfg64=None):
        """-> (rc, out_len, records): rc 0, or QZD_ERR_DSTCAP (-3) with the leading blocks that fit; other codes raise"""
        nb = (n + block_sz - 1) // block_sz
        recs = np.zeros(nb, BLOCKREC_DT)
        ol = C.c_uint64(0)
        rc = self.L.qzd_blocks_compress(self.h, d_src.ptr, n, block_sz, level, thrshold,
                                        C.byref(CrcCfg(*cfg32)) if cfg32 else None, C.byref(CrcCfg(*cfg64)) if cfg64 else None,
                                        d_dst.ptr, d_dst.nbytes if dst_cap is None else dst_cap, recs.ctypes.data, C.byref(ol))
        if rc not in (0, -3):
            self._chk(rc)
        return rc, ol.value, recs

    def blocks_decompress(self, d_comp, comp_len, recs, block_sz, d_out, out_cap=None):
        """-> (rc, out_len, per-block status)"""
        recs = np.ascontiguousarray(recs, dtype=BLOCKREC_DT)
        status = np.zeros(len(recs), np.int32)
        ol = C.c_uint64(0)
        rc = self.L.qzd_blocks_decompress(self.h, d_comp.ptr, comp_len, recs.ctypes.data, len(recs), block_sz, d_out.ptr,
                                          d_out.nbytes if out_cap is None else out_cap, status.ctypes.data, C.byref(ol))
        return rc, ol.value, status

    # -- LZ4
    def lz4_compress_frames(self, d_src, n, d_dst, frame_sz=65536, level=1, hw=False):
        """-> (out_len, per-frame lengths).  level 1-2: liblz4's fast parser, 3-8: LZ4-HC (qzd_lz4hc_*); hw: the hardware
        path's header per frame (frame_sz may then exceed 64 KB: linked blocks)"""
        nfr = max(1, (n + frame_sz - 1) // frame_sz)
        ol = C.c_uint64(0)
        lens = np.zeros(nfr, np.uint32)
        if level >= 3:
            fn = self.L.qzd_lz4hc_compress_frames_hw if hw else self.L.qzd_lz4hc_compress_frames
            self._chk(fn(self.h, d_src.ptr, n, frame_sz, level, d_dst.ptr, d_dst.nbytes, C.byref(ol), lens.ctypes.data))
        else:
            fn = self.L.qzd_lz4_compress_frames_hw if hw else self.L.qzd_lz4_compress_frames
            self._chk(fn(self.h, d_src.ptr, n, frame_sz, d_dst.ptr, d_dst.nbytes, C.byref(ol), lens.ctypes.data))
        return ol.value, lens

    def lz4_compress_linked(self, d_src, n, d_dst, level=1):
        """one call above 64 KB as the ONE frame of linked blocks LZ4F_compressFrame writes for it -> out_len"""
        ol = C.c_uint64(0)
        if level >= 3:
            self._chk(self.L.qzd_lz4hc_compress_linked(self.h, d_src.ptr, n, level, d_dst.ptr, d_dst.nbytes, C.byref(ol)))
        else:
            self._chk(self.L.qzd_lz4_compress_linked(self.h, d_src.ptr, n, d_dst.ptr, d_dst.nbytes, C.byref(ol)))
        return ol.value

    def lz4s_compress_blocks(self, d_src, n, d_dst, block_sz=65536, mini_match=3, level=1, dst_cap=None):
        """every block_sz bytes one LZ4s block (u32le size, LZ77 sequences) -> (out_len, per-block lengths with the size word)"""
        nb = (n + block_sz - 1) // block_sz
        ol = C.c_uint64(0)
        lens = np.zeros(max(nb, 1), np.uint32)
        self._chk(self.L.qzd_lz4s_compress_blocks(self.h, d_src.ptr, n, block_sz, mini_match, level, d_dst.ptr,
                                                  d_dst.nbytes if dst_cap is None else dst_cap, C.byref(ol), lens.ctypes.data))
        return ol.value, lens[:nb]

    def zstd_compress_frames(self, d_src, n, d_dst, block_sz=65536, mini_match=3, level=1, dst_cap=None, seq_flags=None,
                             parse_depth=None):
        """every block_sz bytes one zstd frame (the LZ4s parse, entropy-coded on the device) -> (out_len, per-frame lengths).
        seq_flags (the bits of include/qzamd_zstd_seq.h): through qzd_zstd_compress_frames_ex; parse_depth (the depth of
        include/qzamd_zstd_parse.h): through qzd_zstd_compress_frames_parse, with seq_flags or 0"""
        nb = (n + block_sz - 1) // block_sz
        ol = C.c_uint64(0)
        lens = np.zeros(max(nb, 1), np.uint32)
        args = (self.h, d_src.ptr, n, block_sz, mini_match, level, d_dst.ptr, d_dst.nbytes if dst_cap is None else dst_cap,
                C.byref(ol), lens.ctypes.data)
        if parse_depth is not None:
            self._chk(self.L.qzd_zstd_compress_frames_parse(*args, seq_flags or 0, parse_depth))
        else:
            self._chk(self.L.qzd_zstd_compress_frames(*args) if seq_flags is None else self.L.qzd_zstd_compress_frames_ex(*args, seq_flags))
        return ol.value, lens[:nb]

    def zstd_encode_frames(self, d_literals, d_seqs, desc, d_dst, dst_cap=None, seq_flags=None):
        """the entropy stage alone: desc = uint32 x 3 per frame (content size, records, literals), d_seqs the records (uint32 x
        3: literal length, match length, offset), d_literals their literals -> (rc, out_len, per-frame lengths); rc is the
        device layer's (QZD_ERR_PARAM -1, QZD_ERR_DATA -4 for what it refuses).  seq_flags: through qzd_zstd_encode_frames_ex"""
        desc = np.ascontiguousarray(desc, dtype=np.uint32)
        nf = len(desc) // 3
        ol = C.c_uint64(0)
        lens = np.zeros(max(nf, 1), np.uint32)
        args = (self.h, d_literals.ptr, d_seqs.ptr, desc.ctypes.data, nf, d_dst.ptr, d_dst.nbytes if dst_cap is None else dst_cap,
                C.byref(ol), lens.ctypes.data)
        rc = self.L.qzd_zstd_encode_frames(*args) if seq_flags is None else self.L.qzd_zstd_encode_frames_ex(*args, seq_flags)
        return rc, ol.value, lens[:nf]

    LZ4D_ROUTES = {"auto": 0, "wave": 1, "blocks": 2}

    def lz4_decode_route(self, route):
        """how lz4_decompress_frames treats frames above 65571 bytes from now on: "auto", "wave" (every frame on one wave)
        or "blocks" (a wave per block for every frame of independent blocks that qualifies)"""
        self._chk(self.L.qzd_lz4_decode_route(self.h, self.LZ4D_ROUTES[route]))

    def lz4_decompress_frames(self, d_comp, d_out, segs, route=None):
        """segs: list of (in_off, out_off, in_len, out_cap) -> structured results (status, in_used, out_len).  route: see
        lz4_decode_route; given here it holds for this call and for those after it"""
        if route is not None:
            self.lz4_decode_route(route)
        sa = np.array([tuple(s) for s in segs], dtype=LZ4SEG_DT)
        res = np.zeros(len(segs), LZ4RES_DT)
        self._chk(self.L.qzd_lz4_decompress_frames(self.h, d_comp.ptr, d_out.ptr, sa.ctypes.data, len(segs), res.ctypes.data))
        return res

    ZSTDD_ROUTES = {"auto": 0, "frame": 1, "blocks": 2}

    def zstd_decode_route(self, route):
        """which frames zstd_decompress_frames reads a block per lane group when their block counts are given: "auto" (2
        blocks and more), "frame" (none) or "blocks" (every frame with a count)"""
        self._chk(self.L.qzd_zstd_decode_route(self.h, self.ZSTDD_ROUTES[route]))

    def zstd_decompress_frames(self, d_comp, d_out, segs, nblocks=None, route=None):
        """zstd and skippable frames; segs: list of (in_off, out_off, in_len, out_cap) -> structured results (status,
        in_used, out_len): 0, or -1 malformed, -2 beyond out_cap, -3 truncated, -4 content checksum, -5 unsupported.
        nblocks: per frame its block count or 0 (qzd_zstd_decompress_frames_ex; -6 for a frame whose count is wrong);
        route: see zstd_decode_route; given here it holds for this call and for those after it"""
        if route is not None:
            self.zstd_decode_route(route)
        sa = np.array([tuple(s) for s in segs], dtype=LZ4SEG_DT)
        res = np.zeros(len(segs), LZ4RES_DT)
        if nblocks is None:
            self._chk(self.L.qzd_zstd_decompress_frames(self.h, d_comp.ptr, d_out.ptr, sa.ctypes.data, len(segs), res.ctypes.data))
        else:
            nb = np.ascontiguousarray(nblocks, dtype=np.uint32)
            assert len(nb) == len(segs)
            self._chk(self.L.qzd_zstd_decompress_frames_ex(self.h, d_comp.ptr, d_out.ptr, sa.ctypes.data, len(segs), res.ctypes.data,
                                                           nb.ctypes.data))
        return res

    def zstd_count_blocks(self, d_comp, segs):
        """the block counts of resident frames, 0 where a frame has no last block (qzd_zstd_count_blocks)"""
        sa = np.array([tuple(s) for s in segs], dtype=LZ4SEG_DT)
        nb = np.zeros(max(len(segs), 1), np.uint32)
        self._chk(self.L.qzd_zstd_count_blocks(self.h, d_comp.ptr, sa.ctypes.data, len(segs), nb.ctypes.data))
        return nb[:len(segs)]

    def inflate_timing(self):
        ms = (C.c_float * 4)()
        self.L.qzd_last_inflate_timing(self.h, C.byref(ms))
        return list(ms)


def max_deflate_len(n, chunk_sz=65536):
    """worst-case raw stream size for n bytes (stored blocks + markers)"""
    nchunks = max(1, (n + chunk_sz - 1) // chunk_sz)
    return n + nchunks * (5 * (chunk_sz // 32767 + 2) + 16) + 64


def lz4s_bound(n, block_sz=65536):
    """what the LZ4s blocks of n bytes can grow to (qzd_lz4s_bound): per block of c bytes 4 + c + c/255 + 4*ceil(c/65535) + 16"""
    return int(load().qzd_lz4s_bound(n, block_sz))


def zstd_bound(n, block_sz=65536):
    """what the zstd frames of n bytes can grow to (qzd_zstd_bound): per chunk of c bytes c + 12"""
    return int(load().qzd_zstd_bound(n, block_sz))
