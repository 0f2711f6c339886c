"""deflate_compression_amd -- MI355X-native DEFLATE encoder (host mirror of the
reference's codec API, src/include/deflate_ext.h of mparker97/deflate_compression).

The compute path is libdmx.so (hand-written HIP kernels for gfx950 behind a C ABI,
include/dmx.h).  This module is a thin ctypes layer:

    deflate_compress(fd_in, fd_out, fd_stats=-1, sw=32768, ops=0) -> int
        deflate_ext.h:17 / deflate_compress.c:362 -- 0 or -E_* (no exceptions, like C)
    deflate_decompress(data, ops=0) -> bytes
        deflate_ext.h:16 -- raises DeflateError(code) on a negative return
    compress(data, sw=32768, max_chain=0) -> bytes        host buffer convenience (gzip=True: a .gz member,
                                                          bgzf=True: BGZF, a gzip member per block)
    bgzf_index(z) / inflate_bgzf_gpu(z)                   a BGZF file's members, decoded in parallel on the GPU
    decompress_bgzf(z) -> bytes                           the same from and to host buffers (any BGZF file)
    bgzf_index_gpu(zt) / inflate_bgzf_tensor(zt)          a BGZF file in device memory: indexed and decoded where it lies
    bgzf_read_ranges(zt, ranges) / bgzf_pread(zt, off, n) byte ranges of such a file: only the members they touch are decoded
    inflate_batch(streams)                                many independent zlib / gzip / raw DEFLATE streams, side by side
                                                          (zdict=: preset dictionaries, zlib's FDICT / inflateSetDictionary)
    inflate_parallel_plan_host(z)                         ONE zlib / gzip / raw stream cut at true block starts (host)
    inflate_parallel(zt)                                  ... cut on the device and decoded a wave per chunk, in one pass
    inflate_parallel_multi_plan_host(z)                   ONE .gz file of many members (cat a.gz b.gz, WARC) cut the same way (host)
    inflate_parallel_multi(zt) -> (out, members)          ... decoded in one pass on the device, every member's CRC-32 checked there
    inflate_parallel_multi_plan_async / inflate_parallel_multi_decode_async
                                                          ... the two device calls on caller-owned tensors, for a graph
                                                          (records: ParMultiStatus, PMember / PMEMBER_DTYPE)
    zindex_build(z) -> ZIndex                             ONE such stream indexed once on the host: seek points with windows
    inflate_parallel_indexed(zt) -> (out, ZIndex)         ... decoded in one pass on the device, which leaves the same index there
    inflate_indexed(zt, ix) / zindex_pread(zt, ix, off, n)  ... then decoded a wave per point, or only the points a range touches
    zip_index(z) / zip_index_gpu(zt) -> ZipIndex          a ZIP archive's entries, found on the host / where it lies on the device
    zip_read(zt, index, which) / unzip(z)                 ... any selection of them decoded in one chain of launches, CRC-32 checked
    compress_batch(bufs)                                  many independent buffers into as many streams, in one chain of launches
    Encoder                                               device-resident encodes

There is no CPU fallback: if libdmx.so is missing the import of this module fails,
and on a machine without an MI355X every encode fails with -E_NEXIST.
"""
from __future__ import annotations

import ctypes
import os
import struct

__all__ = [
    "DeflateError", "Opts", "Result", "Encoder", "lib", "compress", "deflate_compress",
    "deflate_decompress", "max_compressed", "adler32_combine", "gen_text", "gen_random",
    "COMPRESS_STATS", "E", "DMX_F_HEADER", "DMX_F_TRAILER", "DMX_F_FINAL", "DMX_ZLIB", "DMX_F_LAZY", "DMX_F_EXACT_SORT", "DMX_F_SPLIT", "DMX_F_DICT", "DMX_F_STORE_CHECK", "DMX_F_DEEP", "DMX_F_GZIP", "DMX_GZIP", "DMX_F_BGZF", "DMX_BGZF", "DMX_F_FDICT", "crc32_combine", "crc32_geometry", "bgzf_index", "inflate_bgzf_gpu", "decompress_bgzf", "bgzf_index_gpu", "inflate_bgzf_tensor", "crc32_ranges", "DMX_BGZF_MAX_ISIZE", "inflate_gpu", "inflate_gpu_chained", "ref_estimates",
    "bgzf_read_ranges", "bgzf_pread", "bgzf_voffset", "bgzf_read_ranges_async", "ranges_geometry", "BRange", "RangesStatus",
    "DMX_RANGES_VIRTUAL",
    "inflate_batch", "inflate_batch_async", "BStream", "BResult", "BatchStatus", "BRESULT_DTYPE",
    "DMX_BATCH_AUTO", "DMX_BATCH_ZLIB", "DMX_BATCH_GZIP", "DMX_BATCH_RAW", "DMX_BATCH_MEASURE",
    "inflate_batch_dict_async", "inflate_dict_host", "BDict", "DMX_BATCH_NODICT",
    "compress_batch", "compress_batch_async", "encode_batch_blocks", "EStream", "EResult", "EBatchStatus", "ERESULT_DTYPE",
    "compress_batch_dict_async",
    "inflate_parallel_plan_host", "PChunk", "ParStatus", "PCHUNK_DTYPE",
    "inflate_parallel", "inflate_parallel_plan_async", "inflate_parallel_decode_async",
    "PMember", "PMEMBER_DTYPE", "ParMultiStatus", "inflate_parallel_multi_plan_host", "inflate_parallel_multi_plan_async",
    "inflate_parallel_multi_decode_async", "inflate_parallel_multi",
    "ZIndex", "ZIndexStatus", "zindex_build", "inflate_points_async", "inflate_indexed", "zindex_read_ranges", "zindex_pread",
    "DMX_ZINDEX_WINDOW", "DMX_ZINDEX_DEF_SPAN", "DMX_ZINDEX_MAX_SPAN",
    "zindex_from_parallel_async", "inflate_parallel_indexed",
    "ZipEntryDTYPE", "ZipStatus", "ZipIndex", "zip_index", "zip_index_gpu", "zip_index_async", "zip_read_async", "zip_read",
    "unzip", "DMX_ZIP_VERIFY",
]

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdmx.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "dmx.h")

DEFLATE_NULLTERM = 1
DMX_F_HEADER, DMX_F_TRAILER, DMX_F_FINAL = 1, 2, 4
DMX_ZLIB = 7
DMX_F_LAZY = 8
DMX_F_EXACT_SORT = 16
DMX_F_SPLIT = 32
DMX_F_DICT = 64
DMX_F_STORE_CHECK = 128
DMX_F_DEEP = 256
DMX_F_GZIP = 512
DMX_GZIP = DMX_ZLIB | DMX_F_GZIP
DMX_F_BGZF = 1024
DMX_BGZF = DMX_F_BGZF | DMX_F_FINAL
DMX_F_FDICT = 2048
DMX_BGZF_MAX_ISIZE = 65536
DMX_RANGES_VIRTUAL = 1
DMX_BATCH_AUTO, DMX_BATCH_ZLIB, DMX_BATCH_GZIP, DMX_BATCH_RAW = 0, 1, 2, 3
DMX_BATCH_MEASURE = 16
DMX_BATCH_NODICT = 0xFFFFFFFF
DMX_ZIP_VERIFY = 1
DMX_ZINDEX_WINDOW = 32768
DMX_ZINDEX_DEF_SPAN = 256 << 10
DMX_ZINDEX_MAX_SPAN = 1 << 30
_M = 1 << 24
# src/include/global_errors.h:24-35 and src/include/deflate_errors.h:9-22
E = {
    "E_LEN": 1, "E_MALLOC": 2, "E_FORK": 3, "E_PIPE": 4, "E_CRC": 5, "E_SZ": 6, "E_EXIST": 7,
    "E_NEXIST": 8, "E_NONULL": 9, "E_RANGE": 10, "E_INVAL": 11, "E_RESERV": 12,
    "E_HUFAMB": _M + 1, "E_HUFINV": _M + 2, "E_HUFVAL": _M + 3, "E_HUFDIS": _M + 4,
    "E_ZADL32": _M + 5, "E_ZHEAD": _M + 6, "E_ZFCHCK": _M + 7, "E_ZCMPMT": _M + 8,
    "E_ZSLWIN": _M + 9, "E_ZPDICT": _M + 10, "E_ZBSZ": _M + 11, "E_ZNLEN": _M + 12,
    "E_ZINV": _M + 13, "E_ZBTYPE": _M + 14, "E_DEVICE": _M + 64,
}
_ENAME = {v: k for k, v in E.items()}

# struct compress_stats (deflate_ext.h:19-31): six little-endian int32
COMPRESS_STATS = struct.Struct("<6i")


class DeflateError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        super().__init__(f"{what or 'dmx'} failed: -{_ENAME.get(-code, str(-code))} ({code})")


class Opts(ctypes.Structure):
    _fields_ = [("sw", ctypes.c_int32), ("max_chain", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("deep_chain", ctypes.c_int32), ("dict", ctypes.c_void_p), ("dict_len", ctypes.c_uint64)]


class Result(ctypes.Structure):
    _fields_ = [("out_len", ctypes.c_uint64), ("end_bits", ctypes.c_uint64), ("n", ctypes.c_uint64),
                ("ntokens", ctypes.c_uint64), ("adler", ctypes.c_uint32), ("status", ctypes.c_int32),
                ("nblocks", ctypes.c_uint32), ("nstored", ctypes.c_uint32), ("nfixed", ctypes.c_uint32),
                ("ndynamic", ctypes.c_uint32), ("nsortfallback", ctypes.c_uint32),
                ("nsortfallback_total", ctypes.c_uint32)]


class FdStats(ctypes.Structure):
    _fields_ = [("chunks", ctypes.c_uint64), ("bytes_in", ctypes.c_uint64), ("bytes_out", ctypes.c_uint64),
                ("wall_ms", ctypes.c_double), ("read_ms", ctypes.c_double), ("h2d_ms", ctypes.c_double),
                ("encode_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double), ("write_ms", ctypes.c_double)]


class BRange(ctypes.Structure):
    """dmx_brange: one (offset, length) request of dmx_bgzf_read_ranges_async"""
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64)]


class RangesStatus(ctypes.Structure):
    """dmx_bgzf_ranges_status: the 32-byte device record of dmx_bgzf_read_ranges_async"""
    _fields_ = [("status", ctypes.c_int32), ("nmembers", ctypes.c_uint32), ("out_len", ctypes.c_uint64),
                ("scratch_len", ctypes.c_uint64), ("bad", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class BStream(ctypes.Structure):
    """dmx_bstream: one stream of dmx_inflate_batch_async -- its input range and its output window"""
    _fields_ = [("in_off", ctypes.c_uint64), ("in_len", ctypes.c_uint64), ("out_off", ctypes.c_uint64),
                ("out_cap", ctypes.c_uint64)]


class BResult(ctypes.Structure):
    """dmx_bresult: the 32-byte result of one stream of dmx_inflate_batch_async"""
    _fields_ = [("status", ctypes.c_int32), ("format", ctypes.c_uint32), ("out_len", ctypes.c_uint64),
                ("in_used", ctypes.c_uint64), ("check", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class BatchStatus(ctypes.Structure):
    """dmx_batch_status: the 16-byte summary record of dmx_inflate_batch_async"""
    _fields_ = [("nfailed", ctypes.c_uint32), ("first_bad", ctypes.c_uint32), ("total_out", ctypes.c_uint64)]


class BDict(ctypes.Structure):
    """dmx_bdict: one preset dictionary of dmx_inflate_batch_dict_async -- its range in the dictionary buffer"""
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64)]


class PChunk(ctypes.Structure):
    """dmx_pchunk: one live chunk of dmx_inflate_parallel_plan_host -- its blocks' bits and its output range"""
    _fields_ = [("bit", ctypes.c_uint64), ("end_bit", ctypes.c_uint64), ("out_off", ctypes.c_uint64),
                ("out_len", ctypes.c_uint64)]


class ParStatus(ctypes.Structure):
    """dmx_par_status: the 56-byte record of dmx_inflate_parallel_plan_host"""
    _fields_ = [("status", ctypes.c_int32), ("format", ctypes.c_uint32), ("out_len", ctypes.c_uint64),
                ("in_used", ctypes.c_uint64), ("check", ctypes.c_uint32), ("nchunks", ctypes.c_uint32),
                ("ncand", ctypes.c_uint32), ("nlive", ctypes.c_uint32), ("ndead", ctypes.c_uint32),
                ("gave_up", ctypes.c_uint32), ("work_len", ctypes.c_uint64)]


class PMember(ctypes.Structure):
    """dmx_pmember: one gzip member of a file of many -- where it lies in the file and in the output, its trailer"""
    _fields_ = [("in_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("out_len", ctypes.c_uint64),
                ("crc", ctypes.c_uint32), ("isize", ctypes.c_uint32)]


class ParMultiStatus(ctypes.Structure):
    """dmx_par_multi_status: the 64-byte record of dmx_inflate_parallel_multi_plan_host"""
    _fields_ = [("st", ParStatus), ("nmembers", ctypes.c_uint32), ("bad_member", ctypes.c_uint32)]


class ZIndexStatus(ctypes.Structure):
    """dmx_zindex_status: the 40-byte record of dmx_zindex_build_host"""
    _fields_ = [("status", ctypes.c_int32), ("format", ctypes.c_uint32), ("out_len", ctypes.c_uint64),
                ("in_used", ctypes.c_uint64), ("check", ctypes.c_uint32), ("npoints", ctypes.c_uint32),
                ("span", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ZipStatus(ctypes.Structure):
    """dmx_zip_status: the 40-byte record of dmx_zip_index_host / dmx_zip_index_async"""
    _fields_ = [("status", ctypes.c_int32), ("nentries", ctypes.c_uint32), ("out_len", ctypes.c_uint64),
                ("cd_off", ctypes.c_uint64), ("cd_len", ctypes.c_uint64), ("ncand", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


# numpy's view of dmx_zip_entry records (64 bytes)
ZipEntryDTYPE = [("data_off", "<u8"), ("csize", "<u8"), ("usize", "<u8"), ("out_off", "<u8"), ("hdr_off", "<u8"),
                 ("name_off", "<u8"), ("crc", "<u4"), ("status", "<i4"), ("method", "<u2"), ("flags", "<u2"),
                 ("name_len", "<u2"), ("reserved", "<u2")]

# numpy's view of dmx_pchunk records
PCHUNK_DTYPE = [("bit", "<u8"), ("end_bit", "<u8"), ("out_off", "<u8"), ("out_len", "<u8")]

# numpy's view of dmx_pmember records
PMEMBER_DTYPE = [("in_off", "<u8"), ("out_off", "<u8"), ("out_len", "<u8"), ("crc", "<u4"), ("isize", "<u4")]

# numpy's view of dmx_bresult records
BRESULT_DTYPE = [("status", "<i4"), ("format", "<u4"), ("out_len", "<u8"), ("in_used", "<u8"), ("check", "<u4"),
                 ("reserved", "<u4")]


class EStream(ctypes.Structure):
    """dmx_estream: one buffer of dmx_encode_batch_async -- its input range"""
    _fields_ = [("in_off", ctypes.c_uint64), ("in_len", ctypes.c_uint64)]


class EResult(ctypes.Structure):
    """dmx_eresult: the 32-byte result of one stream of dmx_encode_batch_async"""
    _fields_ = [("status", ctypes.c_int32), ("nblocks", ctypes.c_uint32), ("out_off", ctypes.c_uint64),
                ("out_len", ctypes.c_uint64), ("check", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class EBatchStatus(ctypes.Structure):
    """dmx_ebatch_status: the 32-byte record of a whole dmx_encode_batch_async call"""
    _fields_ = [("status", ctypes.c_int32), ("nfailed", ctypes.c_uint32), ("first_bad", ctypes.c_uint32),
                ("nblocks", ctypes.c_uint32), ("out_len", ctypes.c_uint64), ("in_len", ctypes.c_uint64)]


# numpy's view of dmx_eresult records
ERESULT_DTYPE = [("status", "<i4"), ("nblocks", "<u4"), ("out_off", "<u8"), ("out_len", "<u8"), ("check", "<u4"),
                 ("reserved", "<u4")]


class _StringLen(ctypes.Structure):
    _fields_ = [("str", ctypes.POINTER(ctypes.c_ubyte)), ("len", ctypes.c_size_t)]


_lib = None
_libc = ctypes.CDLL(None)
_libc.free.argtypes = [ctypes.c_void_p]
_libc.free.restype = None


def lib() -> ctypes.CDLL:
    """Load libdmx.so (built by __graft_entry__.build() / `make -C deflate_compression_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (the encoder has no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, i32, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    sig = {
        "deflate_compress": ([ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_ushort, ctypes.c_int], ctypes.c_int),
        "deflate_decompress": ([ctypes.POINTER(_StringLen), ctypes.POINTER(_StringLen), ctypes.c_int], ctypes.c_int),
        "spawn_deflate_compr_t": ([], vp),
        "deflate_compr_init": ([vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_ushort], None),
        "deflate_compr_deinit": ([vp], None),
        "dmx_ctx_create": ([ctypes.c_int, u64, ctypes.POINTER(vp)], ctypes.c_int),
        "dmx_ctx_destroy": ([vp], None),
        "dmx_ctx_reserve": ([vp, u64, i32], ctypes.c_int),
        "dmx_ctx_reserve_flags": ([vp, u64, i32, u32], ctypes.c_int),
        "dmx_fault_set": ([ctypes.c_char_p], ctypes.c_int),
        "dmx_encode_fd_multi": ([ctypes.c_int, ctypes.c_int, ctypes.POINTER(Opts), u64,
                                 ctypes.POINTER(ctypes.c_int), ctypes.c_int], ctypes.c_int),
        "dmx_max_compressed": ([u64, i32], u64),
        "dmx_max_compressed_flags": ([u64, i32, u32], u64),
        "dmx_crc32_async": ([vp, vp, u64, vp, vp], ctypes.c_int),
        "dmx_crc32_blocks_async": ([vp, vp, u64, i32, vp, vp], ctypes.c_int),
        "dmx_bgzf_index": ([vp, u64, vp, vp, u32, u32p, ctypes.POINTER(u64)], ctypes.c_int),
        "dmx_bgzf_index_max": ([vp, u64, u32, vp, vp, u32, u32p, ctypes.POINTER(u64)], ctypes.c_int),
        "dmx_bgzf_decode_host": ([vp, u64, vp, u64, ctypes.POINTER(u64), ctypes.c_int], ctypes.c_int),
        "dmx_crc32_ranges_async": ([vp, u64, vp, u32, vp, vp, vp], ctypes.c_int),
        "dmx_bgzf_index_work": ([u64, u32], u64),
        "dmx_bgzf_index_geometry": ([u32p], None),
        "dmx_bgzf_index_async": ([vp, u64, u32, vp, vp, u32, vp, u64, vp, vp], ctypes.c_int),
        "dmx_bgzf_decode_device": ([vp, u64, vp, u64, ctypes.POINTER(u64), ctypes.c_int, vp], ctypes.c_int),
        "dmx_inflate_members_async": ([vp, u64, vp, u32, vp, u64, vp, vp, vp], ctypes.c_int),
        "dmx_bgzf_ranges_work": ([u32, u32, u32, u64], u64),
        "dmx_bgzf_ranges_geometry": ([u32p, u32p], None),
        "dmx_bgzf_read_ranges_async": ([vp, u64, vp, vp, u32, vp, u32, u32, vp, u64, vp, u32, u64, vp, u64, vp, vp],
                                       ctypes.c_int),
        "dmx_bgzf_read_device": ([vp, u64, vp, vp, u32, vp, u32, u32, vp, u64, vp, ctypes.POINTER(u64), ctypes.c_int, vp],
                                 ctypes.c_int),
        "dmx_inflate_batch_work": ([u32], u64),
        "dmx_inflate_batch_async": ([vp, u64, vp, u32, u32, vp, u64, vp, vp, u64, vp, vp], ctypes.c_int),
        "dmx_inflate_batch_dict_work": ([u32, u32], u64),
        "dmx_inflate_batch_dict_async": ([vp, u64, vp, u32, u32, vp, u64, vp, u32, vp, vp, u64, vp, vp, u64, vp, vp],
                                         ctypes.c_int),
        "dmx_zip_index_host": ([vp, u64, vp, u32, ctypes.POINTER(ZipStatus)], ctypes.c_int),
        "dmx_zip_index_work": ([u64, u32], u64),
        "dmx_zip_index_async": ([vp, u64, vp, u32, vp, u64, vp, vp], ctypes.c_int),
        "dmx_zip_read_work": ([u32], u64),
        "dmx_zip_read_async": ([vp, u64, vp, u32, vp, u32, u32, vp, u64, vp, vp, vp, u64, vp, vp], ctypes.c_int),
        "dmx_zip_index_geometry": ([u32p], None),
        "dmx_zip_read_geometry": ([u32p], None),
        "dmx_inflate_dict_host": ([vp, u64, u32, vp, u64, ctypes.POINTER(vp), ctypes.POINTER(u64), ctypes.POINTER(u64)],
                                  ctypes.c_int),
        "dmx_inflate_parallel_plan_host": ([vp, u64, u32, u32, vp, u32, ctypes.POINTER(ParStatus)], ctypes.c_int),
        "dmx_inflate_parallel_plan_work": ([u64, u32], u64),
        "dmx_inflate_parallel_plan_async": ([vp, u64, u32, u32, vp, u64, vp], ctypes.c_int),
        "dmx_inflate_parallel_work": ([u64, u32], u64),
        "dmx_inflate_parallel_decode_async": ([vp, u64, vp, u64, u32, vp, u64, vp, u64, ctypes.c_int, vp, vp], ctypes.c_int),
        "dmx_inflate_parallel_multi_plan_host": ([vp, u64, u32, u32, vp, u32, vp, u32, ctypes.POINTER(ParMultiStatus)],
                                                 ctypes.c_int),
        "dmx_inflate_parallel_multi_plan_work": ([u64, u32], u64),
        "dmx_inflate_parallel_multi_plan_async": ([vp, u64, u32, u32, vp, u64, vp], ctypes.c_int),
        "dmx_inflate_parallel_multi_work": ([u64, u32, u32], u64),
        "dmx_inflate_parallel_multi_decode_async": ([vp, u64, vp, u64, u32, u32, vp, u64, vp, vp, u64, ctypes.c_int, vp, vp],
                                                    ctypes.c_int),
        "dmx_zindex_build_host": ([vp, u64, u32, u32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                   ctypes.POINTER(ZIndexStatus)], ctypes.c_int),
        "dmx_inflate_points_work": ([u32], u64),
        "dmx_zindex_points_bound": ([u64, u32, u32], u32),
        "dmx_zindex_device_work": ([u64, u32], u64),
        "dmx_zindex_from_parallel_async": ([vp, u64, vp, vp, u64, u32, u32, vp, vp, vp, u32, vp, u64, vp, vp], ctypes.c_int),
        "dmx_zindex_from_chunks_host": ([vp, u32, vp, u64, u32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                         u32p], ctypes.c_int),
        "dmx_inflate_points_async": ([vp, u64, vp, vp, vp, u32, vp, vp, u32, vp, u64, vp, vp, u64, vp, vp], ctypes.c_int),
        "dmx_encode_batch_blocks": ([u64, u32, i32], u32),
        "dmx_encode_batch_bound": ([u64, u32, i32, u32], u64),
        "dmx_ctx_reserve_batch": ([vp, u32, u32, i32, u32], ctypes.c_int),
        "dmx_encode_batch_async": ([vp, vp, u64, vp, u32, u32, ctypes.POINTER(Opts), vp, u64, vp, vp, vp], ctypes.c_int),
        "dmx_encode_batch_dict_bound": ([u64, u32, i32, u32], u64),
        "dmx_encode_batch_dict_geometry": ([u32p], None),
        "dmx_ctx_reserve_batch_dict": ([vp, u32, u32, u32, i32, u32], ctypes.c_int),
        "dmx_encode_batch_dict_async": ([vp, vp, u64, vp, u32, u32, vp, u64, vp, u32, vp, ctypes.POINTER(Opts), vp, u64, vp, vp,
                                         vp], ctypes.c_int),
        "dmx_crc32_combine": ([u32, u32, u64], u32),
        "dmx_crc32_geometry": ([u32p, u32p], None),
        "dmx_fd_last_stats": ([ctypes.POINTER(FdStats)], ctypes.c_int),
        "dmx_encode_async": ([vp, vp, u64, vp, u64, ctypes.POINTER(Opts), vp], ctypes.c_int),
        "dmx_encode_result": ([vp, ctypes.POINTER(Result), vp], ctypes.c_int),
        "dmx_encode_result_async": ([vp, vp, vp], ctypes.c_int),
        "dmx_encode_host": ([vp, u64, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(Opts)], ctypes.c_int),
        "dmx_last_blocks": ([vp, u32p, u8p, u32p, u32], ctypes.c_int),
        "dmx_last_tokens": ([vp, u32, u32p, u32], ctypes.c_int),
        "dmx_last_code_lengths": ([vp, u32, u8p], ctypes.c_int),
        "dmx_last_subblock": ([vp, u32, u32, u32p, u32p, u32p, u8p], ctypes.c_int),
        "dmx_ctx_set_timing": ([vp, ctypes.c_int], ctypes.c_int),
        "dmx_ctx_set_hook": ([vp, ctypes.c_int, ctypes.c_int], ctypes.c_int),
        "dmx_ctx_stage_times": ([vp, ctypes.POINTER(ctypes.c_double), u32p], ctypes.c_int),
        "dmx_adler32_combine": ([u32, u32, u64], u32),
        "dmx_debug_stamps": ([vp, ctypes.POINTER(u64), u32], ctypes.c_int),
        "dmx_block_index": ([vp, vp, u32, vp], ctypes.c_int),
        "dmx_inflate_async": ([vp, u64, vp, u32, vp, u64, vp, vp], ctypes.c_int),
        "dmx_gen_text": ([vp, u64, u64], None),
        "dmx_gen_random": ([vp, u64, u64], None),
        "dmx_inflate_chained_async": ([vp, u64, vp, u32, vp, u64, vp, u64, vp, vp], ctypes.c_int),
        "dmx_inflate_chained_lists": ([vp, u32p, u32, vp], ctypes.c_int),
        "dmx_inflate_chained_work": ([u64, u32], u64),
        "dmx_refest_create": ([], vp),
        "dmx_refest_destroy": ([vp], None),
        "dmx_refest_feed": ([vp, u32p, u32, vp, u32p], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def _check(r: int, what: str) -> None:
    if r != 0:
        raise DeflateError(r, what)


def _buf(data):
    """(ctypes pointer, length, keepalive) for bytes / bytearray / memoryview / numpy."""
    try:
        import numpy as np
        if isinstance(data, np.ndarray):
            a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            return ctypes.c_void_p(a.ctypes.data), a.size, a
    except ImportError:  # pragma: no cover
        pass
    b = bytes(data)
    cb = ctypes.create_string_buffer(b, len(b) or 1)
    return ctypes.cast(cb, ctypes.c_void_p), len(b), cb


def fd_last_stats() -> dict | None:
    """Per-stage busy time of the last single-device fd-path call (dmx_fd_last_stats):
    wall, read, h2d, encode, d2h, write in ms, plus chunks and bytes; None before any."""
    st = FdStats()
    if lib().dmx_fd_last_stats(ctypes.byref(st)) != 0:
        return None
    return {k: (round(getattr(st, k), 3) if isinstance(getattr(st, k), float) else int(getattr(st, k)))
            for k, _ in FdStats._fields_}


def max_compressed(n: int, sw: int = 32768, flags: int = DMX_ZLIB) -> int:
    """Worst-case stream bytes for n input bytes (12 more for the gzip container, DMX_F_GZIP; 4 more
    for a DICTID, DMX_F_FDICT;
    26 more per block and 28 for the end-of-file member under DMX_F_BGZF)."""
    return int(lib().dmx_max_compressed_flags(n, sw, flags))


def compress(data, sw: int = 32768, max_chain: int = 0, flags: int = DMX_ZLIB, lazy: bool = False,
             split: bool = False, dict: bool = False, pre=None, store_check: bool = False,
             deep: bool = False, gzip: bool = False, bgzf: bool = False, fdict: bool = False) -> bytes:
    """Encode a host buffer on the GPU; returns the zlib stream (or raw DEFLATE with flags;
    gzip = a gzip member around the same DEFLATE data, DMX_F_GZIP; bgzf = a gzip member per
    sw block and the end-of-file member, DMX_BGZF -- not with split or dict).
    lazy = f2 lazy parse (DMX_F_LAZY), split = f3 adaptive block splitting (DMX_F_SPLIT),
    dict = f1 cross-block dictionary (DMX_F_DICT; pre = the bytes before `data`),
    store_check = noise blocks stored without a parse (DMX_F_STORE_CHECK),
    deep = adaptive chain depth of small-alphabet blocks (DMX_F_DEEP),
    fdict = with dict and pre: the zlib header names `pre` as the stream's preset dictionary (78 BB
    and the DICTID, DMX_F_FDICT), so zlib.decompressobj(zdict=pre) and inflate_batch(zdict=pre)
    decode it; 1 <= len(pre) <= sw."""
    L = lib()
    p, n, keep = _buf(data)
    if gzip:
        flags |= DMX_F_GZIP
    if bgzf:
        flags |= DMX_BGZF
    if fdict:
        flags |= DMX_F_FDICT
    cap = max_compressed(n, sw, flags)
    out = ctypes.create_string_buffer(cap)
    olen = ctypes.c_uint64(0)
    o = Opts(sw, max_chain, flags | (DMX_F_LAZY if lazy else 0) | (DMX_F_SPLIT if split else 0) |
             (DMX_F_DICT if dict else 0) | (DMX_F_STORE_CHECK if store_check else 0) | (DMX_F_DEEP if deep else 0), 0)
    pk = None
    if dict and pre is not None and len(pre):
        pk = ctypes.create_string_buffer(bytes(pre), len(pre))
        o.dict, o.dict_len = ctypes.cast(pk, ctypes.c_void_p), len(pre)
    _check(L.dmx_encode_host(p, n, out, cap, ctypes.byref(olen), ctypes.byref(o)), "dmx_encode_host")
    del keep, pk
    return out.raw[:olen.value]


def deflate_compress(fd_in: int, fd_out: int, fd_stats: int = -1, sw: int = 32768, ops: int = 0) -> int:
    """deflate_ext.h:17 -- returns 0 or -E_* exactly like the C entry point."""
    return int(lib().deflate_compress(fd_in, fd_out, fd_stats, sw & 0xFFFF, ops))


def deflate_decompress(data, ops: int = 0) -> bytes:
    """deflate_ext.h:16 -- inflate a zlib stream or a gzip member; raises DeflateError on -E_*."""
    L = lib()
    b = bytes(data)
    src = (ctypes.c_ubyte * max(len(b), 1)).from_buffer_copy(b or b"\0")
    cin = _StringLen(ctypes.cast(src, ctypes.POINTER(ctypes.c_ubyte)), len(b))
    cout = _StringLen()
    r = L.deflate_decompress(ctypes.byref(cout), ctypes.byref(cin), ops)
    if r != 0:
        raise DeflateError(r, "deflate_decompress")
    n = cout.len + (1 if ops & DEFLATE_NULLTERM else 0)
    res = ctypes.string_at(cout.str, n)
    _libc.free(ctypes.cast(cout.str, ctypes.c_void_p))
    return res


def inflate_gpu(z, out_cap: int, index=None, nblk: int = 0, stream=None):
    """Inflate on the GPU (csrc/dmx_inflate_dev.hip).  z: uint8 CUDA tensor.  index=None:
    z is a whole zlib stream, decoded in one workgroup with the Adler-32 check.  index:
    the encoder's block index (Encoder.block_index), every block decoded in parallel.
    Returns (uint8 tensor of out_len bytes, status) -- status 0 or -E_*."""
    import numpy as np
    import torch
    L = lib()
    dev = z.device
    out = torch.empty(max(out_cap, 1), dtype=torch.uint8, device=dev)
    st = torch.zeros(16, dtype=torch.uint8, device=dev)
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    r = L.dmx_inflate_async(z.data_ptr(), z.numel(), index.data_ptr() if index is not None else None,
                            nblk, out.data_ptr(), out_cap, st.data_ptr(), s)
    _check(r, "dmx_inflate_async")
    torch.cuda.synchronize(dev)
    h = st.cpu().numpy()
    status = int(np.frombuffer(h[:4].tobytes(), np.int32)[0])
    olen = int(np.frombuffer(h[8:16].tobytes(), np.uint64)[0])
    return out[:olen], status


def bgzf_index(z, max_member: int = 32768):
    """The members of a BGZF file in host memory (dmx_bgzf_index_max): (index, crcs, total) -- index
    a uint8 numpy array of nblk x 24 B dmx_iblock records (one per member with data: the first
    bit of its DEFLATE data, output offset and length), crcs the members' stored CRC-32s
    (uint32[nblk]), total the decoded length.  A member of more than max_member input bytes raises
    DeflateError(-E_RANGE): the default 32768 is what inflate_gpu's indexed mode takes, 65536
    (DMX_BGZF_MAX_ISIZE) is every member the format allows, htslib's 65280-byte blocks included
    (inflate_bgzf_gpu, dmx_inflate_members_async).  Pure host code: no GPU needed."""
    import numpy as np
    L = lib()
    p, n, keep = _buf(z)
    nb, tot = ctypes.c_uint32(0), ctypes.c_uint64(0)
    r = L.dmx_bgzf_index_max(p, n, max_member, None, None, 0, ctypes.byref(nb), ctypes.byref(tot))
    if r != 0 and r != -E["E_SZ"]:
        raise DeflateError(r, "dmx_bgzf_index")
    idx = np.zeros(max(nb.value, 1) * 24, np.uint8)
    crc = np.zeros(max(nb.value, 1), np.uint32)
    _check(L.dmx_bgzf_index_max(p, n, max_member, ctypes.c_void_p(idx.ctypes.data), ctypes.c_void_p(crc.ctypes.data),
                                nb.value, ctypes.byref(nb), ctypes.byref(tot)), "dmx_bgzf_index")
    del keep
    return idx[:nb.value * 24], crc[:nb.value], int(tot.value)


def _inflate_status(st):
    """(status, out_len) of a 16-byte dmx_inflate_status CUDA tensor"""
    import numpy as np
    h = st.cpu().numpy()
    return int(np.frombuffer(h[:4].tobytes(), np.int32)[0]), int(np.frombuffer(h[8:16].tobytes(), np.uint64)[0])


def crc32_ranges(t, index, nblk: int, stream=None):
    """CRC-32 of the nblk ranges [out_off, out_off + out_len) of a uint8 CUDA tensor that a
    device index lists (a uint8 CUDA tensor of nblk x 24 B dmx_iblock records; out_len 0..65536,
    any order, any offset), computed on the device in one launch (dmx_crc32_ranges_async): an
    int32 CUDA tensor of nblk words (view as uint32 on the host).  An entry outside the tensor or
    longer than 65536 raises DeflateError(-E_RANGE)."""
    import torch
    w = torch.zeros(max(nblk, 1), dtype=torch.int32, device=t.device)
    st = torch.zeros(16, dtype=torch.uint8, device=t.device)
    s = stream if stream is not None else torch.cuda.current_stream(t.device).cuda_stream
    n = t.numel()
    with torch.cuda.device(t.device):
        _check(lib().dmx_crc32_ranges_async(ctypes.c_void_p(t.data_ptr() if n else 0), n, ctypes.c_void_p(index.data_ptr()),
                                            nblk, ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(st.data_ptr()),
                                            ctypes.c_void_p(s)), "dmx_crc32_ranges_async")
        torch.cuda.synchronize(t.device)
    status, _ = _inflate_status(st)
    if status:
        raise DeflateError(status, "dmx_crc32_ranges_async")
    return w[:nblk]


def inflate_bgzf_gpu(z, verify: bool = True, encoder=None):
    """Inflate a BGZF file (host bytes) on the GPU, every member in parallel: the host index with
    the format's own bound on a member (bgzf_index(z, 65536): htslib's 65280-byte blocks, short
    and empty members in any mix), then dmx_inflate_members_async -- the indexed decode and, with
    `verify`, the CRC-32 of every decoded member compared on the device against its stored value:
    DeflateError(-E_CRC) on a mismatch, the decode's status where the decode failed.
    encoder: an Encoder whose device to use (cuda:0 otherwise).  Returns a uint8 CUDA tensor."""
    import numpy as np
    import torch
    idx, crcs, total = bgzf_index(z, DMX_BGZF_MAX_ISIZE)
    nblk = crcs.size
    dev = torch.device(f"cuda:{encoder.device if encoder is not None else 0}")
    if nblk == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    b = bytes(z) if not isinstance(z, np.ndarray) else z
    zt = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)
    ix = torch.from_numpy(idx.copy()).to(dev)
    want = torch.from_numpy(crcs.view(np.int32).copy()).to(dev)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    st = torch.zeros(16, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().dmx_inflate_members_async(ctypes.c_void_p(zt.data_ptr()), zt.numel(), ctypes.c_void_p(ix.data_ptr()),
                                               nblk, ctypes.c_void_p(out.data_ptr()), total,
                                               ctypes.c_void_p(want.data_ptr() if verify else 0),
                                               ctypes.c_void_p(st.data_ptr()), ctypes.c_void_p(s)),
               "dmx_inflate_members_async")
        torch.cuda.synchronize(dev)
    status, olen = _inflate_status(st)
    if status:
        raise DeflateError(status, "inflate_bgzf_gpu")
    if olen != total:
        raise DeflateError(-E["E_LEN"], "inflate_bgzf_gpu")
    return out


def decompress_bgzf(z, verify: bool = True) -> bytes:
    """Decompress a BGZF file (host bytes) on the GPU into host bytes (dmx_bgzf_decode_host): any
    member the format allows, with `verify` every member's CRC-32 checked on the device
    (DeflateError(-E_CRC)).  An empty file, or one of empty members only, gives b""."""
    L = lib()
    p, n, keep = _buf(z)
    olen = ctypes.c_uint64(0)
    r = L.dmx_bgzf_decode_host(p, n, None, 0, ctypes.byref(olen), 1 if verify else 0)   # the decoded length
    if r != -E["E_SZ"]:
        _check(r, "dmx_bgzf_decode_host")
        return b""
    out = ctypes.create_string_buffer(olen.value)
    _check(L.dmx_bgzf_decode_host(p, n, out, olen.value, ctypes.byref(olen), 1 if verify else 0), "dmx_bgzf_decode_host")
    del keep
    return out.raw[:olen.value]


def bgzf_index_gpu(zt, max_member: int = DMX_BGZF_MAX_ISIZE, cap: int | None = None, stream=None):
    """The members of a BGZF file in device memory, found on the device (dmx_bgzf_index_async): zt is
    a uint8 CUDA tensor, any alignment.  Returns (index, crcs, nblk, total) as dmx_bgzf_index_max
    gives them for the same bytes -- index a uint8 CUDA tensor of nblk x 24 B dmx_iblock records,
    crcs an int32 CUDA tensor of the members' stored CRC-32s (view as uint32 on the host), input
    for dmx_inflate_members_async -- and raises DeflateError with the walk's status for a file that
    does not index.  cap: room for that many entries (-E_SZ where the file has more); by default
    as many as the work buffer has candidates.  The work buffer holds zt.numel() // 256 + 1024
    candidates; a file whose data spells more member headers than that is indexed once more with
    the number the first pass reports.  Synchronises the stream to read the 24-byte record."""
    import numpy as np
    import torch
    L = lib()
    dev = zt.device
    n = zt.numel()
    if n and (zt.dtype != torch.uint8 or not zt.is_cuda or not zt.is_contiguous()):
        raise ValueError("bgzf_index_gpu takes a contiguous uint8 CUDA tensor")
    max_cand = n // 256 + 1024
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        for attempt in (0, 1):
            room = max_cand if cap is None else cap
            wb = int(L.dmx_bgzf_index_work(n, max_cand))
            work = torch.empty(wb, dtype=torch.uint8, device=dev)
            index = torch.empty(max(room, 1) * 24, dtype=torch.uint8, device=dev)
            crcs = torch.empty(max(room, 1), dtype=torch.int32, device=dev)
            st = torch.empty(24, dtype=torch.uint8, device=dev)
            _check(L.dmx_bgzf_index_async(ctypes.c_void_p(zt.data_ptr() if n else 0), n, max_member,
                                          ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(crcs.data_ptr()), room,
                                          ctypes.c_void_p(work.data_ptr()), wb, ctypes.c_void_p(st.data_ptr()),
                                          ctypes.c_void_p(s)), "dmx_bgzf_index_async")
            if stream is not None:
                torch.cuda.synchronize(dev)
            h = st.cpu().numpy()
            status, nblk, ncand = int(h[:4].view(np.int32)[0]), int(h[4:8].view(np.uint32)[0]), int(h[16:20].view(np.uint32)[0])
            total = int(h[8:16].view(np.uint64)[0])
            if status == -E["E_SZ"] and nblk == 0 and ncand > max_cand and attempt == 0:
                max_cand = ncand
                continue
            break
    if status:
        raise DeflateError(status, "dmx_bgzf_index_async")
    return index[:nblk * 24], crcs[:nblk], nblk, total


def inflate_bgzf_tensor(zt, verify: bool = True):
    """Inflate a BGZF file that lies in device memory (a uint8 CUDA tensor, any alignment) into a new
    uint8 CUDA tensor on the same device, without a copy of the file to the host
    (dmx_bgzf_decode_device): the device index, then every member decoded in parallel and, with
    `verify`, its CRC-32 checked on the device (DeflateError(-E_CRC)).  Two calls, as
    decompress_bgzf: the first for the decoded length.  An empty file, or one of empty members
    only, gives an empty tensor."""
    import torch
    L = lib()
    dev = zt.device
    n = zt.numel()
    if n and (zt.dtype != torch.uint8 or not zt.is_cuda or not zt.is_contiguous()):
        raise ValueError("inflate_bgzf_tensor takes a contiguous uint8 CUDA tensor")
    olen = ctypes.c_uint64(0)
    with torch.cuda.device(dev):
        s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        zp = ctypes.c_void_p(zt.data_ptr() if n else 0)
        r = L.dmx_bgzf_decode_device(zp, n, None, 0, ctypes.byref(olen), 1 if verify else 0, s)   # the decoded length
        if r != -E["E_SZ"]:
            _check(r, "dmx_bgzf_decode_device")
            return torch.empty(0, dtype=torch.uint8, device=dev)
        out = torch.empty(olen.value, dtype=torch.uint8, device=dev)
        _check(L.dmx_bgzf_decode_device(zp, n, ctypes.c_void_p(out.data_ptr()), olen.value, ctypes.byref(olen),
                                        1 if verify else 0, s), "dmx_bgzf_decode_device")
    return out


def bgzf_voffset(member_off: int, within: int) -> int:
    """The BGZF virtual offset of byte `within` of the data of the member at file offset member_off
    (what .bai / .tbi indexes store): member_off << 16 | within."""
    if not (0 <= within < 65536 and 0 <= member_off < 1 << 48):
        raise ValueError("a virtual offset holds a 48-bit file offset and a 16-bit offset in the member")
    return (member_off << 16) | within


def ranges_geometry() -> tuple[int, int]:
    """(members, ranges) per scan tile of dmx_bgzf_read_ranges_async (tests straddle them)"""
    t, r = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib().dmx_bgzf_ranges_geometry(ctypes.byref(t), ctypes.byref(r))
    return int(t.value), int(r.value)


def _ranges_tensor(ranges, dev):
    """ranges as an int64 CUDA tensor of shape (n, 2): the bits of n dmx_brange records"""
    import numpy as np
    import torch
    if isinstance(ranges, torch.Tensor):
        if ranges.dim() != 2 or ranges.shape[1] != 2 or ranges.dtype not in (torch.int64, torch.uint64):
            raise ValueError("ranges is an (n, 2) int64 / uint64 array of (off, len)")
        return ranges.view(torch.int64).contiguous().to(dev)
    a = np.asarray(ranges, dtype=np.uint64) if not isinstance(ranges, np.ndarray) else ranges
    if a.size == 0:
        a = a.reshape(0, 2)
    if a.ndim != 2 or a.shape[1] != 2 or a.dtype not in (np.int64, np.uint64):
        raise ValueError("ranges is an (n, 2) int64 / uint64 array of (off, len)")
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to(dev)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def bgzf_read_ranges_async(zt, index, crcs, nblk: int, ranges, nranges: int, flags: int, out, out_cap: int, offsets,
                           max_members: int, scratch_bytes: int, work, status, stream=None) -> int:
    """dmx_bgzf_read_ranges_async on caller-owned CUDA tensors, enqueued on `stream` (the current
    one by default) with no synchronisation, so it can be captured into a graph: index / crcs / nblk
    as bgzf_index_gpu returns them (crcs None: no verification), ranges an (n, 2) int64 tensor,
    offsets an int64 tensor of nranges + 1, work a uint8 tensor of lib().dmx_bgzf_ranges_work(...)
    bytes (256-byte aligned), status a 32-byte uint8 tensor (RangesStatus).  Returns the call's own
    return code; the outcome is in the record."""
    import torch
    dev = work.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_bgzf_read_ranges_async(_ptr(zt), zt.numel(), _ptr(index), _ptr(crcs), nblk, _ptr(ranges), nranges,
                                                flags, _ptr(out), out_cap, ctypes.c_void_p(offsets.data_ptr()), max_members,
                                                scratch_bytes, ctypes.c_void_p(work.data_ptr()), work.numel(),
                                                ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(s))


def _ranges_record(status) -> RangesStatus:
    """the record of a 32-byte status tensor (synchronises)"""
    return RangesStatus.from_buffer_copy(status.cpu().numpy().tobytes())


def bgzf_read_ranges(zt, ranges, index=None, virtual: bool = False, verify: bool = True, info: dict | None = None):
    """Read many ranges of the decoded bytes of a BGZF file that lies in device memory
    (dmx_bgzf_read_ranges_async): zt is a contiguous uint8 CUDA tensor, ranges an (n, 2) int64 /
    uint64 array or CUDA tensor of (off, len) -- clipped as pread clips, in any order, overlapping
    or repeated -- or with `virtual` of (BGZF virtual offset, len), see bgzf_voffset.  index: the
    tuple bgzf_index_gpu(zt) returns, built here when None (pass it when reading more than once).
    Only the members the ranges touch are decoded, once each, and with `verify` their CRC-32s are
    checked on the device.  Returns (out, offsets): the bytes packed back to back as a uint8 CUDA
    tensor and an int64 CUDA tensor of n + 1 with range q at out[offsets[q]:offsets[q + 1]].
    Raises DeflateError with the record's status; for -E_RANGE the message names the bad range.
    info: a dict that receives nmembers, scratch_len and out_len of the record.  Two enqueues with
    one synchronisation between them: the first plans, its record sizes the second."""
    import torch
    L = lib()
    dev = zt.device
    if zt.numel() and (zt.dtype != torch.uint8 or not zt.is_cuda or not zt.is_contiguous()):
        raise ValueError("bgzf_read_ranges takes a contiguous uint8 CUDA tensor")
    if index is None:
        index = bgzf_index_gpu(zt)
    ix, crcs, nblk, _ = index
    rt = _ranges_tensor(ranges, dev)
    n = rt.shape[0]
    flags = DMX_RANGES_VIRTUAL if virtual else 0
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    st = torch.empty(32, dtype=torch.uint8, device=dev)
    out = torch.empty(0, dtype=torch.uint8, device=dev)
    want = crcs if verify else None
    members, scratch = 0, 0
    for attempt in (0, 1):
        work = torch.empty(int(L.dmx_bgzf_ranges_work(nblk, n, members, scratch)), dtype=torch.uint8, device=dev)
        _check(bgzf_read_ranges_async(zt, ix, want, nblk, rt, n, flags, out, out.numel(), offsets, members, scratch, work, st),
               "dmx_bgzf_read_ranges_async")
        rec = _ranges_record(st)
        if attempt == 0 and rec.status == -E["E_SZ"]:   # planned: size the real call by the record
            members, scratch = rec.nmembers, rec.scratch_len
            out = torch.empty(rec.out_len, dtype=torch.uint8, device=dev)
            continue
        break
    if info is not None:
        info.update(nmembers=rec.nmembers, scratch_len=rec.scratch_len, out_len=rec.out_len)
    if rec.status == -E["E_RANGE"]:
        bad = rt[rec.bad].cpu().numpy().view("uint64")
        raise DeflateError(rec.status, f"bgzf_read_ranges: range {rec.bad} (virtual offset {int(bad[0]):#x}, len {int(bad[1])})")
    if rec.status:
        raise DeflateError(rec.status, "bgzf_read_ranges")
    return out, offsets


def bgzf_pread(zt, off: int, n: int, index=None, verify: bool = True):
    """Bytes [off, off + n) of the decoded bytes of a BGZF file in device memory, clipped at its end
    as pread clips (dmx_bgzf_read_device): a uint8 CUDA tensor.  index: the tuple bgzf_index_gpu(zt)
    returns, built here when None.  Two calls, as inflate_bgzf_tensor: the first for the length."""
    import numpy as np
    import torch
    L = lib()
    dev = zt.device
    if zt.numel() and (zt.dtype != torch.uint8 or not zt.is_cuda or not zt.is_contiguous()):
        raise ValueError("bgzf_pread takes a contiguous uint8 CUDA tensor")
    if index is None:
        index = bgzf_index_gpu(zt)
    ix, crcs, nblk, _ = index
    rt = _ranges_tensor(np.array([[off, n]], dtype=np.uint64), dev)
    offsets = torch.empty(2, dtype=torch.int64, device=dev)
    olen = ctypes.c_uint64(0)
    out = torch.empty(0, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for attempt in (0, 1):
            r = L.dmx_bgzf_read_device(_ptr(zt), zt.numel(), _ptr(ix), _ptr(crcs), nblk, _ptr(rt), 1, 0, _ptr(out), out.numel(),
                                       ctypes.c_void_p(offsets.data_ptr()), ctypes.byref(olen), 1 if verify else 0, s)
            if attempt == 0 and r == -E["E_SZ"]:
                out = torch.empty(olen.value, dtype=torch.uint8, device=dev)
                continue
            break
    _check(r, "dmx_bgzf_read_device")
    return out


_BATCH_FMT = {"auto": DMX_BATCH_AUTO, "zlib": DMX_BATCH_ZLIB, "gzip": DMX_BATCH_GZIP, "raw": DMX_BATCH_RAW}


def inflate_batch_async(zt, streams, nstreams: int, flags: int, out, out_bytes: int, results, work, status, stream=None) -> int:
    """dmx_inflate_batch_async on caller-owned CUDA tensors, enqueued on `stream` (the current one by
    default) with no synchronisation, so it can be captured into a graph: zt the compressed bytes,
    streams an (n, 4) int64 tensor of dmx_bstream records (in_off, in_len, out_off, out_cap), flags a
    DMX_BATCH_* format with or without DMX_BATCH_MEASURE, out the output (None when measuring),
    results a tensor of 32 x nstreams bytes (BResult records), work a uint8 tensor of
    lib().dmx_inflate_batch_work(nstreams) bytes (256-byte aligned), status a 16-byte tensor
    (BatchStatus).  Returns the call's own return code; the outcomes are in the records."""
    import torch
    dev = work.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_inflate_batch_async(_ptr(zt), zt.numel() if zt is not None else 0, _ptr(streams), nstreams, flags,
                                             _ptr(out), out_bytes, ctypes.c_void_p(results.data_ptr()),
                                             ctypes.c_void_p(work.data_ptr()), work.numel(),
                                             ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(s))


def inflate_batch_dict_async(zt, streams, nstreams: int, flags: int, dict_t, dicts, ndicts: int, dict_of, out,
                             out_bytes: int, results, work, status, stream=None) -> int:
    """dmx_inflate_batch_dict_async on caller-owned CUDA tensors, as inflate_batch_async (no
    synchronisation: it can be captured into a graph): dict_t the dictionaries' bytes (uint8), dicts an
    (ndicts, 2) int64 tensor of dmx_bdict records (off, len) into it, dict_of an int32 / uint32 tensor
    with a dictionary index per stream (DMX_BATCH_NODICT, or -1 as int32: none) or None (every stream
    uses dictionary 0), work of lib().dmx_inflate_batch_dict_work(nstreams, ndicts) bytes."""
    import torch
    dev = work.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_inflate_batch_dict_async(_ptr(zt), zt.numel() if zt is not None else 0, _ptr(streams), nstreams, flags,
                                                  _ptr(dict_t), dict_t.numel() if dict_t is not None else 0, _ptr(dicts),
                                                  ndicts, _ptr(dict_of), _ptr(out), out_bytes,
                                                  ctypes.c_void_p(results.data_ptr()), ctypes.c_void_p(work.data_ptr()),
                                                  work.numel(), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(s))


def inflate_dict_host(z, zdict=None, fmt: str = "auto"):
    """One stream on the host with a preset dictionary (dmx_inflate_dict_host): what
    zlib.decompressobj(wbits, zdict=zdict) makes of z -- a zlib stream with FDICT whose DICTID names
    zdict, a zlib stream without FDICT (zdict is ignored), a raw stream (fmt="raw": zdict always
    primes the window) or a gzip member.  zdict=None: no dictionary.  Returns (bytes, in_used);
    raises DeflateError with the stream's status."""
    if fmt not in _BATCH_FMT:
        raise ValueError("fmt is one of " + ", ".join(_BATCH_FMT))
    zp, zn, zk = _buf(z)
    dp, dn, dk = _buf(zdict) if zdict is not None else (ctypes.c_void_p(0), 0, None)
    out, olen, used = ctypes.c_void_p(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    r = lib().dmx_inflate_dict_host(zp, zn, _BATCH_FMT[fmt], dp, dn, ctypes.byref(out), ctypes.byref(olen), ctypes.byref(used))
    del zk, dk
    if r != 0:
        raise DeflateError(r, "dmx_inflate_dict_host")
    res = ctypes.string_at(out, olen.value)
    _libc.free(out)
    return res, int(used.value)


def _batch_dicts(zdict, dicts, dict_of, n: int, dev):
    """(dict_t, dicts_t, ndicts, dict_of_t) on dev from inflate_batch's zdict / dicts / dict_of"""
    import numpy as np
    import torch
    if isinstance(zdict, torch.Tensor):
        if dicts is None:
            raise ValueError("a dictionary tensor comes with dicts, an (n, 2) int64 array of (off, len)")
        if zdict.numel() and (zdict.dtype != torch.uint8 or not zdict.is_cuda or not zdict.is_contiguous()):
            raise ValueError("zdict is a contiguous uint8 CUDA tensor")
        da = np.asarray(dicts.cpu() if isinstance(dicts, torch.Tensor) else dicts).astype(np.int64).reshape(-1, 2)
        dict_t = zdict
    else:
        parts = [bytes(zdict)] if isinstance(zdict, (bytes, bytearray, memoryview)) else [bytes(b) for b in zdict]
        lens = np.array([len(b) for b in parts], dtype=np.int64)
        offs = np.concatenate(([0], np.cumsum(lens)[:-1])) if len(parts) else np.zeros(0, np.int64)
        da = np.stack([offs, lens], axis=1).astype(np.int64).reshape(-1, 2)
        dict_t = torch.frombuffer(bytearray(b"".join(parts) or b"\0"), dtype=torch.uint8).to(dev)[:int(lens.sum())]
    dicts_t = torch.from_numpy(np.ascontiguousarray(da)).to(dev)
    of_t = None
    if dict_of is not None:
        if isinstance(dict_of, torch.Tensor):
            of = dict_of.cpu().numpy().astype(np.int64).reshape(-1)
        else:
            of = np.array([-1 if v is None else int(v) for v in dict_of], dtype=np.int64)
        if of.shape[0] != n:
            raise ValueError("dict_of has one entry per stream")
        of = np.where(of < 0, DMX_BATCH_NODICT, of).astype(np.uint32)
        of_t = torch.from_numpy(of.view(np.int32).copy()).to(dev)
    return dict_t, dicts_t, da.shape[0], of_t


def inflate_batch(z, streams=None, fmt: str = "auto", sizes=None, strict: bool = True, zdict=None, dict_of=None,
                  dicts=None):
    """Inflate many independent zlib streams, gzip members or raw DEFLATE streams on the GPU, side
    by side (dmx_inflate_batch_async): z is a list of bytes-like objects, packed into one device
    tensor here, or a contiguous uint8 CUDA tensor with `streams`, an (n, 2) int64 array of
    (off, len) into it.  fmt: "auto" (1F 8B names a gzip member, anything else a zlib stream),
    "zlib", "gzip" or "raw".  sizes: the decoded lengths where the caller knows them -- one decode
    pass, and a length that is too small shows as -E_SZ; without it a measure pass runs first, an
    exclusive scan of its lengths on the device places the windows, and one synchronisation sizes
    the output.  Returns (out, offsets, results): the decoded bytes packed back to back as a uint8
    CUDA tensor, an int64 CUDA tensor of n + 1 with stream k at out[offsets[k]:offsets[k + 1]] (its
    first results[k].out_len bytes), and a numpy structured array of the BResult records (status,
    format, out_len, in_used, check).  strict: a stream with a status raises DeflateError with the
    status of the lowest such index, which the message names.
    zdict: preset dictionaries (dmx_inflate_batch_dict_async; RFC 1950 FDICT, zlib's zdict=) -- one
    bytes-like object, a list of them, or a contiguous uint8 CUDA tensor with `dicts`, an (n, 2) int64
    array of (off, len) into it.  dict_of: a sequence or tensor with the dictionary index of every
    stream, -1 or None for none; by default every stream uses dictionary 0.  A zlib stream takes its
    dictionary where its header has FDICT and names it (else -E_ZPDICT), a raw stream always, a zlib
    stream without FDICT and a gzip member never.  With zdict=None the call is dmx_inflate_batch_async."""
    import numpy as np
    import torch
    L = lib()
    if fmt not in _BATCH_FMT:
        raise ValueError("fmt is one of " + ", ".join(_BATCH_FMT))
    if zdict is None and (dict_of is not None or dicts is not None):
        raise ValueError("dict_of and dicts come with zdict")
    flags = _BATCH_FMT[fmt]
    if isinstance(z, torch.Tensor):
        if streams is None:
            raise ValueError("a tensor comes with streams, an (n, 2) int64 array of (off, len)")
        if z.numel() and (z.dtype != torch.uint8 or not z.is_cuda or not z.is_contiguous()):
            raise ValueError("inflate_batch takes a contiguous uint8 CUDA tensor")
        zt = z
        sa = np.asarray(streams.cpu() if isinstance(streams, torch.Tensor) else streams).astype(np.int64).reshape(-1, 2)
    else:
        parts = [bytes(b) for b in z]
        lens = np.array([len(b) for b in parts], dtype=np.int64)
        offs = np.concatenate(([0], np.cumsum(lens)[:-1])) if len(parts) else np.zeros(0, np.int64)
        sa = np.stack([offs, lens], axis=1).astype(np.int64).reshape(-1, 2)
        zt = torch.frombuffer(bytearray(b"".join(parts) or b"\0"), dtype=torch.uint8).cuda()
    dev = zt.device
    n = sa.shape[0]
    desc = np.zeros((n, 4), dtype=np.int64)
    desc[:, :2] = sa
    res = torch.zeros(max(n, 1) * 4, dtype=torch.int64, device=dev)
    st = torch.empty(2, dtype=torch.int64, device=dev)
    if zdict is None:
        work = torch.empty(int(L.dmx_inflate_batch_work(n)), dtype=torch.uint8, device=dev)
        what = "dmx_inflate_batch_async"

        def launch(fl, o, ob):
            return inflate_batch_async(zt, dt, n, fl, o, ob, res, work, st)
    else:
        dict_t, dicts_t, nd, of_t = _batch_dicts(zdict, dicts, dict_of, n, dev)
        work = torch.empty(int(L.dmx_inflate_batch_dict_work(n, nd)), dtype=torch.uint8, device=dev)
        what = "dmx_inflate_batch_dict_async"

        def launch(fl, o, ob):
            return inflate_batch_dict_async(zt, dt, n, fl, dict_t, dicts_t, nd, of_t, o, ob, res, work, st)
    measured = None
    if sizes is not None:
        sz = np.asarray(sizes, dtype=np.int64).reshape(-1)
        if sz.shape[0] != n:
            raise ValueError("sizes has one length per stream")
        offsets_h = np.concatenate(([0], np.cumsum(sz))).astype(np.int64)
        desc[:, 2], desc[:, 3] = offsets_h[:-1], sz
        dt = torch.from_numpy(desc).to(dev)
        offsets = torch.from_numpy(offsets_h).to(dev)
        total = int(offsets_h[-1])
    else:
        desc[:, 3] = -1   # UINT64_MAX: no limit
        dt = torch.from_numpy(desc).to(dev)
        _check(launch(flags | DMX_BATCH_MEASURE, None, 0), what)
        measured = res.view(max(n, 1), 4)[:n].clone()
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(measured[:, 1], 0, out=offsets[1:])
        dt[:, 2], dt[:, 3] = offsets[:-1], measured[:, 1]
        total = int(offsets[-1].item())   # the call's one synchronisation before the decode
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    _check(launch(flags, out, total), what)
    rt = res.view(max(n, 1), 4)[:n]
    if measured is not None:
        # a stream the measure pass refused has a window of 0 bytes: its status is the measured one
        rt = torch.where((measured[:, 0] & 0xFFFFFFFF != 0)[:, None], measured, rt)
    results = rt.cpu().numpy().view(np.uint8).reshape(-1).view(BRESULT_DTYPE)
    rec = BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    if strict and rec.nfailed:
        raise DeflateError(int(results["status"][rec.first_bad]), f"inflate_batch: stream {rec.first_bad}")
    return out[:total], offsets, results


# ---- ZIP archives (include/dmx.h: dmx_zip_index_host, dmx_zip_index_async, dmx_zip_read_async) ----

class ZipIndex:
    """The entries of a ZIP archive: `entries` a uint8 CUDA tensor of 64-byte dmx_zip_entry records
    (None for an index made on the host until zip_read uploads it), `host` the same records as a
    numpy structured array (ZipEntryDTYPE), `status` the ZipStatus record.  len() is the number of
    entries held; names are fetched lazily -- only the central directory's bytes go to the host --
    and decoded as zipfile decodes them: UTF-8 where flag bit 11 is set, else cp437."""

    def __init__(self, host, status: ZipStatus, entries=None, source=None):
        self.host = host
        self.status = status
        self.entries = entries
        self._source = source   # the archive: bytes-like or a CUDA tensor
        self._names = None
        self._by_name = None

    def __len__(self) -> int:
        return int(self.host.shape[0])

    @property
    def out_len(self) -> int:
        return int(self.status.out_len)

    @property
    def names(self) -> list:
        if self._names is None:
            a, n = int(self.status.cd_off), int(self.status.cd_len)
            src = self._source
            if hasattr(src, "is_cuda"):
                cd = src[a:a + n].cpu().numpy().tobytes()
            else:
                cd = bytes(memoryview(src)[a:a + n])
            out = []
            for e in self.host:
                o = int(e["name_off"]) - a
                raw = cd[o:o + int(e["name_len"])]
                out.append(raw.decode("utf-8") if int(e["flags"]) & 0x800 else raw.decode("cp437"))
            self._names = out
        return self._names

    def find(self, name: str) -> int:
        """the index of the last entry with this name (zipfile's rule for duplicates); KeyError if none"""
        if self._by_name is None:
            self._by_name = {nm: i for i, nm in enumerate(self.names)}
        return self._by_name[name]

    def device_entries(self, dev):
        import torch
        if self.entries is None or self.entries.device != dev:
            import numpy as np
            raw = np.ascontiguousarray(self.host).view(np.uint8).reshape(-1)
            self.entries = torch.from_numpy(raw.copy() if raw.size else np.zeros(64, np.uint8)).to(dev)[:raw.size]
        return self.entries


def zip_index(z, cap: int | None = None) -> ZipIndex:
    """The index of a ZIP archive in host memory (dmx_zip_index_host: no GPU).  Raises DeflateError with
    the file's status (-E_SZ only where cap is given and too small); an entry's own status is in its
    record and fails nothing here."""
    import numpy as np
    L = lib()
    p, n, keep = _buf(z)
    st = ZipStatus()
    if cap is None:
        _check(L.dmx_zip_index_host(p, n, None, 0, ctypes.byref(st)), "dmx_zip_index_host")
        if st.status not in (0, -E["E_SZ"]):
            raise DeflateError(st.status, "dmx_zip_index_host")
        cap = st.nentries
    ent = np.zeros(max(cap, 1), dtype=ZipEntryDTYPE)
    _check(L.dmx_zip_index_host(p, n, ctypes.c_void_p(ent.ctypes.data), cap, ctypes.byref(st)), "dmx_zip_index_host")
    del keep
    if st.status:
        raise DeflateError(st.status, "dmx_zip_index_host")
    return ZipIndex(ent[:st.nentries], st, source=z)


def zip_index_async(zt, entries, cap: int, work, status, stream=None) -> int:
    """dmx_zip_index_async on caller-owned CUDA tensors, enqueued on `stream` (the current one by
    default) with no synchronisation, so it can be captured into a graph: zt the archive (uint8, any
    alignment), entries a uint8 tensor of 64 x cap bytes, work a uint8 tensor of
    lib().dmx_zip_index_work(zt.numel(), max_cand) bytes (256-byte aligned), status a 40-byte uint8
    tensor (ZipStatus).  Returns the call's own return code; the outcome is in the record."""
    import torch
    dev = work.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_zip_index_async(_ptr(zt), zt.numel(), _ptr(entries), cap, ctypes.c_void_p(work.data_ptr()),
                                         work.numel(), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(s))


def zip_read_async(zt, entries, nentries: int, sel, nsel: int, flags: int, out, out_bytes: int, offsets, results, work,
                   status, stream=None) -> int:
    """dmx_zip_read_async on caller-owned CUDA tensors, as zip_index_async (no synchronisation: it can
    be captured into a graph): entries / nentries as an index call wrote them, sel an int32 / uint32
    tensor of nsel selectors or None (all entries, nsel == nentries), flags 0 or DMX_ZIP_VERIFY,
    offsets an int64 tensor of nsel + 1, results a tensor of 32 x nsel bytes (BResult records), work
    a uint8 tensor of lib().dmx_zip_read_work(nsel) bytes, status a 16-byte tensor (BatchStatus)."""
    import torch
    dev = work.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_zip_read_async(_ptr(zt), zt.numel(), _ptr(entries), nentries, _ptr(sel), nsel, flags, _ptr(out),
                                        out_bytes, ctypes.c_void_p(offsets.data_ptr()), ctypes.c_void_p(results.data_ptr()),
                                        ctypes.c_void_p(work.data_ptr()), work.numel(), ctypes.c_void_p(status.data_ptr()),
                                        ctypes.c_void_p(s))


def zip_index_gpu(zt, cap: int | None = None, stream=None, _max_cand: int | None = None) -> ZipIndex:
    """The index of a ZIP archive that lies in device memory, made on the device (dmx_zip_index_async):
    zt is a contiguous uint8 CUDA tensor, any alignment.  The same record and entries as zip_index
    gives for the same bytes.  cap: room for that many entries (-E_SZ where the archive has more);
    by default zt.numel() // 46, which no archive exceeds.  The work buffer holds cap + 1024
    candidates; an archive whose names, extras and comments spell more headers than that is
    indexed once more with the number the first pass reports.  Synchronises the stream to read the
    40-byte record and the entries' host view."""
    import numpy as np
    import torch
    L = lib()
    dev = zt.device
    n = zt.numel()
    if n and (zt.dtype != torch.uint8 or not zt.is_cuda or not zt.is_contiguous()):
        raise ValueError("zip_index_gpu takes a contiguous uint8 CUDA tensor")
    room = n // 46 if cap is None else cap
    max_cand = room + 1024 if _max_cand is None else _max_cand   # (_max_cand: the tests' way into the second pass)
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        for attempt in (0, 1):
            work = torch.empty(int(L.dmx_zip_index_work(n, max_cand)), dtype=torch.uint8, device=dev)
            entries = torch.empty(max(room, 1) * 64, dtype=torch.uint8, device=dev)
            st = torch.empty(40, dtype=torch.uint8, device=dev)
            _check(zip_index_async(zt, entries, room, work, st, s), "dmx_zip_index_async")
            if stream is not None:
                torch.cuda.synchronize(dev)
            rec = ZipStatus.from_buffer_copy(st.cpu().numpy().tobytes())
            if rec.status == -E["E_SZ"] and rec.nentries == 0 and rec.ncand > max_cand and attempt == 0:
                max_cand = rec.ncand
                continue
            break
    if rec.status:
        raise DeflateError(rec.status, "dmx_zip_index_async")
    entries = entries[:rec.nentries * 64]
    host = entries.cpu().numpy().view(ZipEntryDTYPE) if rec.nentries else np.zeros(0, dtype=ZipEntryDTYPE)
    return ZipIndex(host, rec, entries=entries, source=zt)


def zip_read(zt, index: ZipIndex | None = None, which=None, verify: bool = True, strict: bool = True):
    """Decode entries of a ZIP archive that lies in device memory (dmx_zip_read_async): zt a contiguous
    uint8 CUDA tensor, index what zip_index_gpu / zip_index gave for it (made here by default), which
    a list of names or entry numbers in any order, repeats allowed (None: all, in archive order).
    Returns (out, offsets, results): the decoded bytes packed back to back in selection order as a
    uint8 CUDA tensor, an int64 CUDA tensor of n + 1 with selection k at out[offsets[k]:offsets[k + 1]],
    and a numpy structured array of the BResult records (status, format = the method, out_len,
    in_used, check = the stored CRC-32).  verify: every entry's CRC-32 is checked on the device
    (-E_CRC).  The output's size comes from the index's host view, so the read itself makes no
    synchronisation before its results are fetched.  strict: an entry with a status raises
    DeflateError with the status of the lowest such selection, which the message names."""
    import numpy as np
    import torch
    L = lib()
    if zt.numel() and (zt.dtype != torch.uint8 or not zt.is_cuda or not zt.is_contiguous()):
        raise ValueError("zip_read takes a contiguous uint8 CUDA tensor")
    dev = zt.device
    if index is None:
        index = zip_index_gpu(zt)
    ne = len(index)
    if which is None:
        sel_h, sel = np.arange(ne, dtype=np.int64), None
    else:
        sel_h = np.array([index.find(w) if isinstance(w, str) else int(w) for w in which], dtype=np.int64)
        sel = torch.from_numpy(sel_h.astype(np.uint32).view(np.int32).copy()).to(dev) if sel_h.size else None
    n = int(sel_h.size)
    ok = (sel_h >= 0) & (sel_h < ne)
    lens = np.zeros(n, dtype=np.uint64)
    if ne:
        picked = index.host[np.where(ok, sel_h, 0)]
        lens = np.where(ok & (picked["status"] == 0), picked["usize"], 0).astype(np.uint64)
    total = int(lens.sum())
    with torch.cuda.device(dev):
        entries = index.device_entries(dev)
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        res = torch.zeros(max(n, 1) * 4, dtype=torch.int64, device=dev)
        st = torch.empty(2, dtype=torch.int64, device=dev)
        work = torch.empty(int(L.dmx_zip_read_work(n)), dtype=torch.uint8, device=dev)
        if which is not None and n == 0:
            sel = torch.zeros(1, dtype=torch.int32, device=dev)   # (an empty selection is not "all")
        _check(zip_read_async(zt, entries, ne, sel, n, DMX_ZIP_VERIFY if verify else 0, out if total else None, total,
                              offsets, res, work, st), "dmx_zip_read_async")
        results = res.view(max(n, 1), 4)[:n].cpu().numpy().view(np.uint8).reshape(-1).view(BRESULT_DTYPE)
        rec = BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    if strict and rec.nfailed:
        raise DeflateError(int(results["status"][rec.first_bad]), f"zip_read: selection {rec.first_bad}")
    return out[:total], offsets, results


def unzip(z) -> dict:
    """{name: bytes} of a ZIP archive in host memory, decoded on the GPU: the archive is uploaded,
    indexed on the device (zip_index_gpu), every entry decoded and its CRC-32 checked there
    (zip_read), and the bytes brought back.  Raises DeflateError for an archive that does not index
    or an entry that does not decode."""
    import torch
    zb = bytes(z)
    zt = torch.frombuffer(bytearray(zb or b"\0"), dtype=torch.uint8).cuda()[:len(zb)]
    index = zip_index_gpu(zt)
    out, offsets, _ = zip_read(zt, index)
    data = out.cpu().numpy().tobytes()
    off = offsets.cpu().numpy()
    return {nm: data[int(off[k]):int(off[k + 1])] for k, nm in enumerate(index.names)}


def _par_info(rec: ParStatus) -> dict:
    return {f: int(getattr(rec, f)) for f, _ in ParStatus._fields_}


def inflate_parallel_plan_host(z, fmt: str = "auto", chunk_bytes: int | None = None):
    """One zlib stream, gzip member or raw DEFLATE stream cut into chunks that begin at true block
    boundaries, with their output ranges, on the host (dmx_inflate_parallel_plan_host): returns
    (chunks, info) -- the live chunks as a numpy array of PCHUNK_DTYPE records and the record's
    fields as a dict (status included: a stream the plan refuses is not an exception here)."""
    import numpy as np
    if fmt not in _BATCH_FMT:
        raise ValueError("fmt is one of " + ", ".join(_BATCH_FMT))
    zp, zn, zk = _buf(z)
    rec = ParStatus()
    cb = int(chunk_bytes or 0)
    r = lib().dmx_inflate_parallel_plan_host(zp, zn, _BATCH_FMT[fmt], cb, None, 0, ctypes.byref(rec))
    chunks = np.zeros(rec.nlive if r in (0, -E["E_SZ"]) else 0, dtype=PCHUNK_DTYPE)
    if r == -E["E_SZ"]:
        r = lib().dmx_inflate_parallel_plan_host(zp, zn, _BATCH_FMT[fmt], cb, ctypes.c_void_p(chunks.ctypes.data),
                                                 chunks.shape[0], ctypes.byref(rec))
    del zk
    _check(r, "dmx_inflate_parallel_plan_host")
    return chunks, _par_info(rec)


def inflate_parallel_plan_async(zt, fmt: int, chunk_bytes: int, plan, stream=None) -> int:
    """dmx_inflate_parallel_plan_async on caller-owned CUDA tensors, enqueued on `stream` (the current
    one by default) with no synchronisation, so it can be captured into a graph: zt the one stream's
    bytes, fmt a DMX_BATCH_* format, chunk_bytes the cut (0: the default), plan a uint8 tensor of
    lib().dmx_inflate_parallel_plan_work(zt.numel(), chunk_bytes) bytes (256-byte aligned) whose first
    56 bytes receive the ParStatus record.  Returns the call's own return code."""
    import torch
    dev = plan.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_inflate_parallel_plan_async(_ptr(zt), zt.numel() if zt is not None else 0, fmt, chunk_bytes,
                                                     ctypes.c_void_p(plan.data_ptr()), plan.numel(), ctypes.c_void_p(s))


def inflate_parallel_decode_async(zt, plan, max_live: int, out, out_cap: int, work, verify: bool, status, stream=None) -> int:
    """dmx_inflate_parallel_decode_async on caller-owned CUDA tensors, as inflate_parallel_plan_async
    (no synchronisation: both can be captured into one graph): plan as the plan call left it for zt,
    max_live and out_cap the capacities, work a uint8 tensor of at least
    lib().dmx_inflate_parallel_work(out_len, nlive) bytes (256-byte aligned), status a 56-byte tensor
    (ParStatus).  Returns the call's own return code; the outcome is in the record."""
    import torch
    dev = work.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_inflate_parallel_decode_async(_ptr(zt), zt.numel() if zt is not None else 0,
                                                       ctypes.c_void_p(plan.data_ptr()), plan.numel(), max_live, _ptr(out),
                                                       out_cap, ctypes.c_void_p(work.data_ptr()), work.numel(),
                                                       1 if verify else 0, ctypes.c_void_p(status.data_ptr()),
                                                       ctypes.c_void_p(s))


def inflate_parallel(z, fmt: str = "auto", chunk_bytes: int | None = None, verify: bool = True, info: dict | None = None):
    """One zlib stream, gzip member or raw DEFLATE stream that carries no index, decoded in one pass
    on the GPU: z a contiguous uint8 CUDA tensor (or bytes, copied to the device here).  The plan
    (dmx_inflate_parallel_plan_async) cuts it at true block starts, one synchronisation reads its
    56-byte record, the output and the work buffer are allocated, and every live chunk decodes in a
    wave of its own (dmx_inflate_parallel_decode_async).  Where the plan gave the stream up (a chunk
    that expands beyond 4 MiB, too many false block starts) or found one chunk only (stored or fixed
    blocks, nothing to cut), the stream takes the serial route: inflate_batch with that one stream.
    verify: the Adler-32 / CRC-32 and ISIZE are checked on the device.  info (a dict) receives the
    record's fields and route, "parallel" or "serial".  Returns a uint8 CUDA tensor; a stream with a
    status raises DeflateError with it."""
    import torch
    if fmt not in _BATCH_FMT:
        raise ValueError("fmt is one of " + ", ".join(_BATCH_FMT))
    if isinstance(z, torch.Tensor):
        if z.numel() and (z.dtype != torch.uint8 or not z.is_cuda or not z.is_contiguous()):
            raise ValueError("inflate_parallel takes a contiguous uint8 CUDA tensor")
        zt = z
    else:
        b = bytes(z)
        zt = torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).cuda()[:len(b)]
    L = lib()
    dev = zt.device
    cb = int(chunk_bytes or 0)
    pb = int(L.dmx_inflate_parallel_plan_work(zt.numel(), cb))
    if not pb:
        raise ValueError("chunk_bytes is 1024 .. 2^30 (None or 0: the default), the stream at most 0xFFFFFFF0 bytes")
    plan = torch.empty(pb, dtype=torch.uint8, device=dev)
    _check(inflate_parallel_plan_async(zt, _BATCH_FMT[fmt], cb, plan), "dmx_inflate_parallel_plan_async")
    rec = ParStatus.from_buffer_copy(plan[:56].cpu().numpy().tobytes())   # the call's one synchronisation before the decode
    if info is not None:
        info.update(_par_info(rec))
        info["route"] = "parallel"
    if rec.gave_up or (rec.status == 0 and rec.nlive == 1):
        if info is not None:
            info["route"] = "serial"
        out, _, res = inflate_batch(zt, [(0, zt.numel())], fmt=fmt)
        return out[:int(res["out_len"][0])]
    if rec.status:
        raise DeflateError(rec.status, "inflate_parallel")
    out = torch.empty(max(rec.out_len, 1), dtype=torch.uint8, device=dev)
    work = torch.empty(int(rec.work_len), dtype=torch.uint8, device=dev)
    st = torch.empty(7, dtype=torch.int64, device=dev)
    _check(inflate_parallel_decode_async(zt, plan, rec.nlive, out, rec.out_len, work, verify, st),
           "dmx_inflate_parallel_decode_async")
    rec = ParStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    if info is not None:
        info.update(_par_info(rec))
    if rec.status:
        raise DeflateError(rec.status, "inflate_parallel")
    return out[:rec.out_len]


def _par_multi_info(rec: ParMultiStatus) -> dict:
    d = _par_info(rec.st)
    d["nmembers"], d["bad_member"] = int(rec.nmembers), int(rec.bad_member)
    return d


def inflate_parallel_multi_plan_host(z, chunk_bytes: int | None = None):
    """One .gz file of many members (RFC 1952 2.2: `cat a.gz b.gz`, rotated logs, pgzip, WARC) cut into
    chunks that begin at true block boundaries or member starts, on the host
    (dmx_inflate_parallel_multi_plan_host): returns (chunks, members, info) -- the live chunks as
    PCHUNK_DTYPE records, the members as PMEMBER_DTYPE records (in_off, out_off, out_len and the stored
    crc and isize), and the record's fields as a dict (status included, nmembers, bad_member)."""
    import numpy as np
    zp, zn, zk = _buf(z)
    rec = ParMultiStatus()
    cb = int(chunk_bytes or 0)
    r = lib().dmx_inflate_parallel_multi_plan_host(zp, zn, DMX_BATCH_GZIP, cb, None, 0, None, 0, ctypes.byref(rec))
    ok = r in (0, -E["E_SZ"])
    chunks = np.zeros(rec.st.nlive if ok else 0, dtype=PCHUNK_DTYPE)
    members = np.zeros(rec.nmembers if ok else 0, dtype=PMEMBER_DTYPE)
    if r == -E["E_SZ"]:
        r = lib().dmx_inflate_parallel_multi_plan_host(zp, zn, DMX_BATCH_GZIP, cb, ctypes.c_void_p(chunks.ctypes.data),
                                                       chunks.shape[0], ctypes.c_void_p(members.ctypes.data),
                                                       members.shape[0], ctypes.byref(rec))
    del zk
    _check(r, "dmx_inflate_parallel_multi_plan_host")
    return chunks, members, _par_multi_info(rec)


def inflate_parallel_multi_plan_async(zt, fmt: int, chunk_bytes: int, plan, stream=None) -> int:
    """dmx_inflate_parallel_multi_plan_async on caller-owned CUDA tensors, as inflate_parallel_plan_async:
    fmt DMX_BATCH_AUTO or DMX_BATCH_GZIP, plan a uint8 tensor of
    lib().dmx_inflate_parallel_multi_plan_work(zt.numel(), chunk_bytes) bytes (256-byte aligned) whose
    first 64 bytes receive the ParMultiStatus record.  Returns the call's own return code."""
    import torch
    dev = plan.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_inflate_parallel_multi_plan_async(_ptr(zt), zt.numel() if zt is not None else 0, fmt, chunk_bytes,
                                                           ctypes.c_void_p(plan.data_ptr()), plan.numel(), ctypes.c_void_p(s))


def inflate_parallel_multi_decode_async(zt, plan, max_live: int, max_members: int, out, out_cap: int, members, work,
                                        verify: bool, status, stream=None) -> int:
    """dmx_inflate_parallel_multi_decode_async on caller-owned CUDA tensors (no synchronisation: plan and
    decode can be captured into one graph): plan as the plan call left it for zt; max_live, max_members
    and out_cap the capacities; members a tensor of 32 x max_members bytes (8-byte aligned) for the
    PMember records; work a uint8 tensor of at least lib().dmx_inflate_parallel_multi_work(out_len, nlive,
    nmembers) bytes (256-byte aligned); status a 64-byte tensor (ParMultiStatus).  Returns the call's own
    return code; the outcome is in the record."""
    import torch
    dev = work.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_inflate_parallel_multi_decode_async(_ptr(zt), zt.numel() if zt is not None else 0,
                                                             ctypes.c_void_p(plan.data_ptr()), plan.numel(), max_live,
                                                             max_members, _ptr(out), out_cap, _ptr(members),
                                                             ctypes.c_void_p(work.data_ptr()), work.numel(),
                                                             1 if verify else 0, ctypes.c_void_p(status.data_ptr()),
                                                             ctypes.c_void_p(s))


def _multi_serial(zt, info):
    """the serial route of inflate_parallel_multi: member by member through inflate_batch, each stream
    from the member before's in_used on; the same member table, built on the host"""
    import numpy as np
    import torch
    n = zt.numel()
    pos, total, outs, rows = 0, 0, [], []
    while True:
        o, _, res = inflate_batch(zt, [(pos, n - pos)], fmt="gzip", strict=False)
        st = int(res["status"][0])
        if st:
            raise DeflateError(st, f"inflate_parallel_multi: member {len(rows)}")
        olen, used = int(res["out_len"][0]), int(res["in_used"][0])
        isize = int.from_bytes(zt[pos + used - 4:pos + used].cpu().numpy().tobytes(), "little")
        rows.append((pos, total, olen, int(res["check"][0]), isize))
        outs.append(o[:olen])
        total += olen
        pos += used
        if pos + 2 > n or zt[pos:pos + 2].cpu().numpy().tobytes() != b"\x1f\x8b":
            break
    if info is not None:
        info.update(status=0, out_len=total, in_used=pos, check=rows[-1][3], nmembers=len(rows), bad_member=0xFFFFFFFF)
    out = torch.cat(outs) if total else torch.empty(0, dtype=torch.uint8, device=zt.device)
    return out, np.array(rows, dtype=PMEMBER_DTYPE)


def inflate_parallel_multi(z, chunk_bytes: int | None = None, verify: bool = True, info: dict | None = None):
    """One .gz file of many members decoded in one pass on the GPU: z a contiguous uint8 CUDA tensor
    (or bytes, copied to the device here).  As inflate_parallel: the plan
    (dmx_inflate_parallel_multi_plan_async), one synchronisation for its 64-byte record, the
    allocations, the decode (dmx_inflate_parallel_multi_decode_async) -- but the walk goes on behind
    every trailer while 1F 8B follows; anything else there is trailing data and ignored (info["in_used"]
    says where it begins).  verify: every member's CRC-32 and ISIZE are checked on the device; a failure
    raises DeflateError whose message names the member.  Where the plan gave the file up or found one
    live chunk, the file goes member by member through inflate_batch (info["route"] == "serial": slow
    and correct, always verified).  info receives the record's fields and route.  Returns (out,
    members): the members' data back to back as a uint8 CUDA tensor and a numpy array of
    PMEMBER_DTYPE records."""
    import numpy as np
    import torch
    if isinstance(z, torch.Tensor):
        if z.numel() and (z.dtype != torch.uint8 or not z.is_cuda or not z.is_contiguous()):
            raise ValueError("inflate_parallel_multi takes a contiguous uint8 CUDA tensor")
        zt = z
    else:
        b = bytes(z)
        zt = torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).cuda()[:len(b)]
    L = lib()
    dev = zt.device
    cb = int(chunk_bytes or 0)
    pb = int(L.dmx_inflate_parallel_multi_plan_work(zt.numel(), cb))
    if not pb:
        raise ValueError("chunk_bytes is 1024 .. 2^30 (None or 0: the default), the file at most 0xFFFFFFF0 bytes")
    plan = torch.empty(pb, dtype=torch.uint8, device=dev)
    _check(inflate_parallel_multi_plan_async(zt, DMX_BATCH_GZIP, cb, plan), "dmx_inflate_parallel_multi_plan_async")
    rec = ParMultiStatus.from_buffer_copy(plan[:64].cpu().numpy().tobytes())   # the one synchronisation before the decode
    if info is not None:
        info.update(_par_multi_info(rec))
        info["route"] = "parallel"
    if rec.st.gave_up or (rec.st.status == 0 and rec.st.nlive == 1):
        if info is not None:
            info["route"] = "serial"
        return _multi_serial(zt, info)
    if rec.st.status:
        raise DeflateError(rec.st.status, "inflate_parallel_multi")
    out = torch.empty(max(rec.st.out_len, 1), dtype=torch.uint8, device=dev)
    work = torch.empty(int(rec.st.work_len), dtype=torch.uint8, device=dev)
    mem = torch.empty(4 * rec.nmembers, dtype=torch.int64, device=dev)
    st = torch.empty(8, dtype=torch.int64, device=dev)
    _check(inflate_parallel_multi_decode_async(zt, plan, rec.st.nlive, rec.nmembers, out, rec.st.out_len, mem, work, verify, st),
           "dmx_inflate_parallel_multi_decode_async")
    rec = ParMultiStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    if info is not None:
        info.update(_par_multi_info(rec))
    if rec.st.status:
        where = f": member {rec.bad_member}" if rec.bad_member != 0xFFFFFFFF else ""
        raise DeflateError(rec.st.status, "inflate_parallel_multi" + where)
    members = mem.cpu().numpy().view(np.uint8).reshape(-1).view(PMEMBER_DTYPE).copy()
    return out[:rec.st.out_len], members


class ZIndex:
    """The seek-point index of one zlib stream, gzip member or raw DEFLATE stream (zindex_build;
    dmx_zindex_build_host): points, a numpy array of PCHUNK_DTYPE records (bit, end_bit, out_off,
    out_len); adlers, the uint32 Adler-32 of every point's bytes; windows, a uint8 array of
    (npoints, 32768) with the output in front of every point right-aligned in its slot; and format
    (1 zlib, 2 gzip, 3 raw), out_len, in_used (through the trailer), check (the stored Adler-32 /
    CRC-32) and span of the stream.  cuda(device) makes the device copies once per device."""

    def __init__(self, points, adlers, windows, format: int, out_len: int, in_used: int, check: int, span: int):
        import numpy as np
        self.points = np.ascontiguousarray(points, dtype=PCHUNK_DTYPE)
        self.adlers = np.ascontiguousarray(adlers, dtype=np.uint32)
        self.windows = np.ascontiguousarray(windows, dtype=np.uint8).reshape(-1, DMX_ZINDEX_WINDOW)
        if not (self.points.shape[0] == self.adlers.shape[0] == self.windows.shape[0]):
            raise ValueError("points, adlers and windows have one entry per point")
        self.format, self.out_len, self.in_used, self.check, self.span = (int(format), int(out_len), int(in_used),
                                                                          int(check), int(span))
        self._dev = {}

    @property
    def npoints(self) -> int:
        return int(self.points.shape[0])

    @property
    def nbytes(self) -> int:
        return int(self.points.nbytes + self.adlers.nbytes + self.windows.nbytes)

    def cuda(self, device=None):
        """(points, adlers, windows) as CUDA tensors -- (n, 4) int64, (n,) int32 holding the uint32
        bits, (n, 32768) uint8 -- copied on first use and cached per device"""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._dev:
            n = self.npoints
            self._dev[dev] = (torch.from_numpy(self.points.view("<i8").reshape(n, 4).copy()).to(dev),
                              torch.from_numpy(self.adlers.view("<i4").copy()).to(dev),
                              torch.from_numpy(self.windows).to(dev))
        return self._dev[dev]

    def save(self, path) -> None:
        """numpy.savez of the arrays and the record (load: ZIndex.load)"""
        import numpy as np
        meta = np.array([self.format, self.out_len, self.in_used, self.check, self.span], dtype=np.uint64)
        with open(path, "wb") as f:
            np.savez(f, points=self.points, adlers=self.adlers, windows=self.windows, meta=meta)

    @classmethod
    def load(cls, path) -> "ZIndex":
        import numpy as np
        with np.load(path, allow_pickle=False) as f:
            meta = [int(v) for v in f["meta"]]
            return cls(f["points"], f["adlers"], f["windows"], *meta)


def zindex_build(z, fmt: str = "auto", span: int | None = None) -> ZIndex:
    """Index one zlib stream, gzip member or raw DEFLATE stream that carries no index of its own, on
    the host (dmx_zindex_build_host; no GPU): one serial decode, a seek point at the first block
    boundary every `span` bytes of output (default 256 KiB; 1: behind every block that produced
    output), each with its bit offset, its output range, the Adler-32 of its bytes and the 32 KiB of
    output in front of it.  The trailer is checked here.  A stream deflate_decompress refuses raises
    DeflateError with the same status.  Points fall on block boundaries only: a stream that is one
    block is one point.  Pay once, then inflate_indexed / zindex_read_ranges / zindex_pread."""
    import numpy as np
    if fmt not in _BATCH_FMT:
        raise ValueError("fmt is one of " + ", ".join(_BATCH_FMT))
    sp = int(span or 0)
    if sp < 0 or sp > DMX_ZINDEX_MAX_SPAN:
        raise ValueError("span is 1 .. 2^30 (None or 0: the default)")
    zp, zn, zk = _buf(z)
    rec = ZIndexStatus()
    pts, adl, win = ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0)
    r = lib().dmx_zindex_build_host(zp, zn, _BATCH_FMT[fmt], sp, ctypes.byref(pts), ctypes.byref(adl), ctypes.byref(win),
                                    ctypes.byref(rec))
    del zk
    _check(r, "dmx_zindex_build_host")
    if rec.status:
        raise DeflateError(rec.status, "dmx_zindex_build_host")
    try:
        n = rec.npoints
        points = np.frombuffer(ctypes.string_at(pts, 32 * n), dtype=PCHUNK_DTYPE).copy()
        adlers = np.frombuffer(ctypes.string_at(adl, 4 * n), dtype=np.uint32).copy()
        windows = np.ctypeslib.as_array(ctypes.cast(win, ctypes.POINTER(ctypes.c_uint8)),
                                        shape=(n, DMX_ZINDEX_WINDOW)).copy()
    finally:
        for p in (pts, adl, win):
            _libc.free(p)
    return ZIndex(points, adlers, windows, rec.format, rec.out_len, rec.in_used, rec.check, rec.span)


def zindex_from_parallel_async(plan, dec_status, out, out_cap: int, max_live: int, span: int, points, adlers, windows,
                               max_points: int, work, status, stream=None) -> int:
    """dmx_zindex_from_parallel_async on caller-owned CUDA tensors, enqueued on `stream` (the current
    one by default) behind inflate_parallel_decode_async with no synchronisation, so plan, decode and
    index can be captured into one graph: plan, out and dec_status (the decode's 56-byte record) as
    those calls left them, out_cap and max_live the decode's capacities, span 0 for the default;
    points 32 x max_points bytes, adlers 4 x max_points, windows 32768 x max_points; work a uint8 tensor
    of lib().dmx_zindex_device_work(out_cap, max_points) bytes (256-byte aligned); status a 40-byte
    tensor (ZIndexStatus).  Returns the call's own return code; the outcome is in the record."""
    import torch
    dev = work.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_zindex_from_parallel_async(_ptr(plan), plan.numel() if plan is not None else 0, _ptr(dec_status),
                                                    _ptr(out), out_cap, max_live, span, _ptr(points), _ptr(adlers),
                                                    _ptr(windows), max_points, ctypes.c_void_p(work.data_ptr()), work.numel(),
                                                    _ptr(status), ctypes.c_void_p(s))


def inflate_parallel_indexed(z, fmt: str = "auto", chunk_bytes: int | None = None, span: int | None = None,
                             verify: bool = True, info: dict | None = None):
    """inflate_parallel that also leaves the stream's seek-point index: returns (out, ZIndex).  The
    plan, its one synchronisation, the allocations and the decode are inflate_parallel's; the index
    call (dmx_zindex_from_parallel_async) follows on the same stream, sized by
    dmx_zindex_points_bound, its record is the one copy that is waited for (after -E_SZ the call runs
    once more with the npoints it names), and the index is copied to the host for the ZIndex, whose
    per-device cache is seeded with the device tensors: inflate_indexed, zindex_read_ranges and
    zindex_pread then upload nothing.  A point begins at the first chunk boundary `span` bytes of
    output behind the point before (default 256 KiB).  Where inflate_parallel takes the serial route
    (the plan gave the stream up, or found one chunk), out comes from that route and the index from
    zindex_build on the stream's bytes copied to the host.  info (a dict) receives the plan's and the
    decode's fields, route as inflate_parallel, index_route "device" or "host", and npoints."""
    if fmt not in _BATCH_FMT:
        raise ValueError("fmt is one of " + ", ".join(_BATCH_FMT))
    sp = int(span or 0)
    if sp < 0 or sp > DMX_ZINDEX_MAX_SPAN:
        raise ValueError("span is 1 .. 2^30 (None or 0: the default)")
    import numpy as np
    import torch
    if isinstance(z, torch.Tensor):
        if z.numel() and (z.dtype != torch.uint8 or not z.is_cuda or not z.is_contiguous()):
            raise ValueError("inflate_parallel_indexed takes a contiguous uint8 CUDA tensor")
        zt = z
    else:
        b = bytes(z)
        zt = torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).cuda()[:len(b)]
    L = lib()
    dev = zt.device
    cb = int(chunk_bytes or 0)
    pb = int(L.dmx_inflate_parallel_plan_work(zt.numel(), cb))
    if not pb:
        raise ValueError("chunk_bytes is 1024 .. 2^30 (None or 0: the default), the stream at most 0xFFFFFFF0 bytes")
    plan = torch.empty(pb, dtype=torch.uint8, device=dev)
    _check(inflate_parallel_plan_async(zt, _BATCH_FMT[fmt], cb, plan), "dmx_inflate_parallel_plan_async")
    rec = ParStatus.from_buffer_copy(plan[:56].cpu().numpy().tobytes())   # the one synchronisation before the decode
    if info is not None:
        info.update(_par_info(rec))
        info["route"], info["index_route"] = "parallel", "device"
    if rec.gave_up or (rec.status == 0 and rec.nlive == 1):
        if info is not None:
            info["route"], info["index_route"] = "serial", "host"
        out, _, res = inflate_batch(zt, [(0, zt.numel())], fmt=fmt)
        ix = zindex_build(zt.cpu().numpy(), fmt=fmt, span=sp)
        if info is not None:
            info["npoints"] = ix.npoints
        return out[:int(res["out_len"][0])], ix
    if rec.status:
        raise DeflateError(rec.status, "inflate_parallel_indexed")
    out = torch.empty(max(rec.out_len, 1), dtype=torch.uint8, device=dev)
    work = torch.empty(int(rec.work_len), dtype=torch.uint8, device=dev)
    st = torch.empty(7, dtype=torch.int64, device=dev)
    _check(inflate_parallel_decode_async(zt, plan, rec.nlive, out, rec.out_len, work, verify, st),
           "dmx_inflate_parallel_decode_async")
    cap = int(L.dmx_zindex_points_bound(rec.out_len, rec.nlive, sp))
    zst = torch.empty(5, dtype=torch.int64, device=dev)
    for attempt in (0, 1):
        pts = torch.empty((cap, 4), dtype=torch.int64, device=dev)
        adl = torch.empty(cap, dtype=torch.int32, device=dev)
        win = torch.empty((cap, DMX_ZINDEX_WINDOW), dtype=torch.uint8, device=dev)
        zwork = torch.empty(int(L.dmx_zindex_device_work(rec.out_len, cap)), dtype=torch.uint8, device=dev)
        _check(zindex_from_parallel_async(plan, st, out, rec.out_len, rec.nlive, sp, pts, adl, win, cap, zwork, zst),
               "dmx_zindex_from_parallel_async")
        zrec = ZIndexStatus.from_buffer_copy(zst.cpu().numpy().tobytes())
        if attempt == 0 and zrec.status == -E["E_SZ"] and zrec.npoints > cap:
            cap = int(zrec.npoints)
            continue
        break
    if info is not None:
        info.update({f: int(getattr(zrec, f)) for f, _ in ZIndexStatus._fields_ if f != "reserved"})
    if zrec.status:
        raise DeflateError(zrec.status, "inflate_parallel_indexed")
    n = int(zrec.npoints)
    pts, adl, win = pts[:n], adl[:n], win[:n]
    ix = ZIndex(pts.cpu().numpy().view(np.uint8).reshape(-1).view(PCHUNK_DTYPE), adl.cpu().numpy().view(np.uint32),
                win.cpu().numpy(), zrec.format, zrec.out_len, zrec.in_used, zrec.check, zrec.span)
    ix._dev[torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())] = (pts, adl, win)
    return out[:zrec.out_len], ix


def inflate_points_async(zt, points, adlers, windows, npoints: int, sel, dst_off, nsel: int, out, out_bytes: int, results,
                         work, status, stream=None) -> int:
    """dmx_inflate_points_async on caller-owned CUDA tensors, enqueued on `stream` (the current one by
    default) with no synchronisation, so it can be captured into a graph: zt the compressed bytes;
    points / adlers / windows as ZIndex.cuda() returns them (adlers None: no verification); sel an
    int32 tensor of nsel point numbers or None (entry e is point e); dst_off an int64 tensor of nsel
    offsets into out or None (the points' own out_off); results 32 x nsel bytes (BResult records);
    work a uint8 tensor of lib().dmx_inflate_points_work(nsel) bytes (256-byte aligned); status a
    16-byte tensor (BatchStatus).  Returns the call's own return code; the outcomes are in the records."""
    import torch
    dev = work.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_inflate_points_async(_ptr(zt), zt.numel() if zt is not None else 0, _ptr(points), _ptr(adlers),
                                              _ptr(windows), npoints, _ptr(sel), _ptr(dst_off), nsel, _ptr(out), out_bytes,
                                              ctypes.c_void_p(results.data_ptr()), ctypes.c_void_p(work.data_ptr()),
                                              work.numel(), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(s))


def _points_decode(zt, index: ZIndex, sel, dst, total: int, verify: bool, what: str):
    """decode the points `sel` (numpy, None: all) of index to `dst` (numpy offsets, None: their own
    out_off) of a fresh tensor of `total` bytes; raises for the first entry with a status"""
    import numpy as np
    import torch
    if zt.numel() and (zt.dtype != torch.uint8 or not zt.is_cuda or not zt.is_contiguous()):
        raise ValueError(what + " takes a contiguous uint8 CUDA tensor")
    dev = zt.device
    pt, at, wt = index.cuda(dev)
    n = index.npoints if sel is None else int(sel.shape[0])
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    if n == 0:
        return out[:total]
    st = torch.empty(2, dtype=torch.int64, device=dev)
    res = torch.empty(4 * n, dtype=torch.int64, device=dev)
    work = torch.empty(int(lib().dmx_inflate_points_work(n)), dtype=torch.uint8, device=dev)
    sel_t = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel, dtype=np.uint32).view(np.int32).copy()).to(dev)
    dst_t = None if dst is None else torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int64)).to(dev)
    _check(inflate_points_async(zt, pt, at if verify else None, wt, index.npoints, sel_t, dst_t, n, out, total, res, work, st),
           "dmx_inflate_points_async")
    rec = BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    if rec.nfailed:
        bad = res.view(n, 4)[rec.first_bad].cpu().numpy().view(np.uint8).view(BRESULT_DTYPE)
        k = rec.first_bad if sel is None else int(sel[rec.first_bad])
        raise DeflateError(int(bad["status"][0]), f"{what}: point {k}")
    return out[:total]


def inflate_indexed(zt, index: ZIndex, verify: bool = True):
    """The whole output of an indexed stream that lies in device memory (dmx_inflate_points_async):
    zt a contiguous uint8 CUDA tensor with the stream zindex_build indexed, every point a wave of its
    own, all in parallel.  verify: every point's Adler-32 is compared on the device.  Returns a uint8
    CUDA tensor of index.out_len bytes; raises DeflateError with the status of the first bad point."""
    return _points_decode(zt, index, None, None, index.out_len, verify, "inflate_indexed")


_GATHER_CHUNK = 1 << 22


def zindex_read_ranges(zt, index: ZIndex, ranges, verify: bool = True):
    """Many ranges of the decoded bytes of an indexed stream in device memory: ranges is an (n, 2)
    array of (off, len), in any order, overlapping or repeated; only the points they touch are
    decoded, once each, back to back into a scratch tensor, and the bytes asked for are gathered from
    it.  Returns (out, offsets) as bgzf_read_ranges: the bytes packed back to back as a uint8 CUDA
    tensor and an int64 CUDA tensor of n + 1 with range q at out[offsets[q]:offsets[q + 1]].  An empty
    range and one that ends at out_len are legal; one that reaches beyond out_len is a ValueError.
    Device memory: the scratch tensor (the touched points, whole), the output, and at most 128 MiB of
    index tensors for the gather, which runs over groups of ranges of 4 MiB."""
    import numpy as np
    import torch
    a = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    off, ln = a[:, 0], a[:, 1]
    if a.size and (off.min() < 0 or ln.min() < 0 or int((off + ln).max()) > index.out_len):
        raise ValueError(f"a range lies outside the {index.out_len} decoded bytes")
    dev = zt.device
    offsets_h = np.concatenate(([0], np.cumsum(ln))).astype(np.int64)
    total = int(offsets_h[-1])
    offsets = torch.from_numpy(offsets_h).to(dev)
    if total == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), offsets
    po = index.points["out_off"].astype(np.int64)
    live = ln > 0
    first = np.searchsorted(po, off[live], side="right") - 1            # the point that holds the first byte
    lastp = np.searchsorted(po, off[live] + ln[live] - 1, side="right") - 1   # ... and the last
    touched = np.zeros(index.npoints + 1, dtype=np.int64)
    np.add.at(touched, first, 1)
    np.add.at(touched, lastp + 1, -1)
    sel = np.nonzero(np.cumsum(touched[:-1]) > 0)[0]
    plen = index.points["out_len"][sel].astype(np.int64)
    dst = np.concatenate(([0], np.cumsum(plen)))
    scratch = _points_decode(zt, index, sel, dst[:-1], int(dst[-1]), verify, "zindex_read_ranges")
    # where the points' bytes lie in the scratch: output offset o of point sel[j] is at dst[j] + o - out_off
    shift = np.zeros(index.npoints, dtype=np.int64)
    shift[sel] = dst[:-1] - po[sel]
    src0 = np.zeros(a.shape[0], dtype=np.int64)
    src0[live] = off[live] + shift[first]   # (touched points are consecutive in the scratch along a range)
    # the gather, in groups of ranges of at most _GATHER_CHUNK bytes: the index tensors of a group are
    # about 32 bytes per byte gathered, so they stay below 128 MiB whatever is asked for; a range longer
    # than that is one slice copy
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    q, nr = 0, a.shape[0]
    while q < nr:
        if ln[q] >= _GATHER_CHUNK:
            out[offsets_h[q]:offsets_h[q + 1]] = scratch[src0[q]:src0[q] + ln[q]]
            q += 1
            continue
        e = int(np.searchsorted(offsets_h, offsets_h[q] + _GATHER_CHUNK, side="right")) - 1   # offsets_h[e] - offsets_h[q] <= the chunk
        ln_t = torch.from_numpy(ln[q:e].copy()).to(dev)
        nb = int(offsets_h[e] - offsets_h[q])
        if nb:
            rel = torch.from_numpy(src0[q:e] - (offsets_h[q:e] - offsets_h[q])).to(dev)   # source minus place in the group
            idx = torch.repeat_interleave(rel, ln_t) + torch.arange(nb, dtype=torch.int64, device=dev)
            out[offsets_h[q]:offsets_h[e]] = scratch[idx]
        q = e
    return out, offsets


def zindex_pread(zt, index: ZIndex, off: int, n: int, verify: bool = True):
    """Bytes [off, off + n) of the decoded bytes of an indexed stream in device memory: a uint8 CUDA
    tensor.  Only the points the range touches are decoded.  A range beyond out_len is a ValueError."""
    return zindex_read_ranges(zt, index, [[off, n]], verify)[0]


_EBATCH_FMT = {"zlib": DMX_ZLIB, "gzip": DMX_GZIP, "raw": DMX_F_FINAL}


def encode_batch_blocks(lens, sw: int = 32768) -> int:
    """The exact block count of a batch whose lengths are known: the sum of max(1, ceil(len / sw))
    (an empty stream has one empty block, which carries its framing)."""
    sw = sw or 32768
    return int(sum(max(1, -(-int(n) // sw)) for n in lens))


def compress_batch_async(encoder, t_in, streams, nstreams: int, max_blocks: int, out, out_cap: int, results, status,
                         opts: Opts | None = None, stream=None) -> int:
    """dmx_encode_batch_async on caller-owned CUDA tensors, enqueued on `stream` (the current one by
    default) with no synchronisation, so it can be captured into a graph: t_in the input bytes,
    streams an (n, 2) int64 tensor of dmx_estream records (in_off, in_len), max_blocks the capacity in
    blocks (encode_batch_blocks, or lib().dmx_encode_batch_blocks), out the packed output of out_cap
    bytes, results a tensor of 32 x nstreams bytes (EResult records), status a 32-byte tensor
    (EBatchStatus).  The encoder must be reserved (Encoder.reserve_batch).  Where the current stream is
    the legacy default stream (handle 0) the call runs on the encoder's own stream, as
    Encoder.encode_async does: the caller orders it against the tensors' producers and consumers.
    Returns the call's own return code; the outcomes are in the records."""
    import torch
    dev = out.device
    o = opts or encoder.opts
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_encode_batch_async(encoder._ctx, _ptr(t_in), t_in.numel() if t_in is not None else 0,
                                            _ptr(streams), nstreams, max_blocks, ctypes.byref(o),
                                            ctypes.c_void_p(out.data_ptr()), out_cap,
                                            ctypes.c_void_p(results.data_ptr()), ctypes.c_void_p(status.data_ptr()),
                                            ctypes.c_void_p(s))


def compress_batch_dict_async(encoder, t_in, streams, nstreams: int, max_blocks: int, dict_t, dicts, ndicts: int, dict_of,
                              out, out_cap: int, results, status, opts: Opts | None = None, stream=None) -> int:
    """dmx_encode_batch_dict_async on caller-owned CUDA tensors, as compress_batch_async (no
    synchronisation: it can be captured into a graph): dict_t the dictionaries' bytes (uint8), dicts an
    (ndicts, 2) int64 tensor of dmx_bdict records (off, len) into it, dict_of an int32 / uint32 tensor
    with a dictionary index per stream (DMX_BATCH_NODICT, or -1 as int32: none) or None (every stream
    uses dictionary 0).  opts.flags holds DMX_F_DICT.  The encoder must be reserved
    (Encoder.reserve_batch_dict)."""
    import torch
    dev = out.device
    o = opts or encoder.opts
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return lib().dmx_encode_batch_dict_async(encoder._ctx, _ptr(t_in), t_in.numel() if t_in is not None else 0,
                                                 _ptr(streams), nstreams, max_blocks, _ptr(dict_t),
                                                 dict_t.numel() if dict_t is not None else 0, _ptr(dicts), ndicts,
                                                 _ptr(dict_of), ctypes.byref(o), ctypes.c_void_p(out.data_ptr()), out_cap,
                                                 ctypes.c_void_p(results.data_ptr()), ctypes.c_void_p(status.data_ptr()),
                                                 ctypes.c_void_p(s))


def compress_batch(bufs, streams=None, fmt: str = "zlib", sw: int = 32768, max_chain: int = 0, lazy: bool = False,
                   flags: int = 0, encoder=None, strict: bool = True, zdict=None, dict_of=None, fdict: bool = True):
    """Compress many independent buffers into as many independent zlib streams, gzip members or raw
    DEFLATE streams on the GPU, in one chain of launches (dmx_encode_batch_async): bufs is a list of
    bytes-like objects, packed into one device tensor here, or a contiguous uint8 CUDA tensor with
    `streams`, an (n, 2) int64 array of (off, len) into it.  fmt: "zlib", "gzip" or "raw"; flags: more
    parse / block options (DMX_F_DEEP, DMX_F_STORE_CHECK, DMX_F_EXACT_SORT).  Stream k's bytes are what
    a single encode of buffer k gives with the same options.  Returns (out, offsets, results): the
    streams packed back to back as a uint8 CUDA tensor, an int64 CUDA tensor of n + 1 with stream k at
    out[offsets[k]:offsets[k + 1]], and a numpy structured array of the EResult records (status,
    nblocks, out_off, out_len, check).  One synchronisation.  strict: a stream with a status, or a
    status of the whole call, raises DeflateError (a stream's names the lowest such index).
    zdict: preset dictionaries (dmx_encode_batch_dict_async) -- one bytes-like object or a list of them;
    dict_of: the dictionary index of every stream, -1 or None for none (by default every stream uses
    dictionary 0), as in inflate_batch.  Stream k is then what a single encode of buffer k against its
    dictionary gives.  fmt is "zlib" or "raw"; fdict (zlib only): the streams that name a dictionary
    carry FDICT and its DICTID, for zlib.decompressobj(zdict=) and inflate_batch(zdict=); fdict=False
    writes 78 9C headers over the same history, which only a decoder that is given the dictionary by
    other means can read.  Without zdict the call is dmx_encode_batch_async, exactly as before."""
    import numpy as np
    import torch
    L = lib()
    if fmt not in _EBATCH_FMT:
        raise ValueError("fmt is one of " + ", ".join(_EBATCH_FMT))
    if zdict is None and dict_of is not None:
        raise ValueError("dict_of comes with zdict")
    if zdict is not None and fmt == "gzip":
        raise ValueError("a gzip member has no preset dictionary: fmt is zlib or raw with zdict")
    if isinstance(bufs, torch.Tensor):
        if streams is None:
            raise ValueError("a tensor comes with streams, an (n, 2) int64 array of (off, len)")
        if bufs.numel() and (bufs.dtype != torch.uint8 or not bufs.is_cuda or not bufs.is_contiguous()):
            raise ValueError("compress_batch takes a contiguous uint8 CUDA tensor")
        tin = bufs
        sa = np.asarray(streams.cpu() if isinstance(streams, torch.Tensor) else streams).astype(np.int64).reshape(-1, 2)
    else:
        parts = [bytes(b) for b in bufs]
        lens = np.array([len(b) for b in parts], dtype=np.int64)
        offs = np.concatenate(([0], np.cumsum(lens)[:-1])) if len(parts) else np.zeros(0, np.int64)
        sa = np.stack([offs, lens], axis=1).astype(np.int64).reshape(-1, 2)
        dev0 = f"cuda:{encoder.device}" if encoder is not None else "cuda"
        tin = torch.frombuffer(bytearray(b"".join(parts) or b"\0"), dtype=torch.uint8).to(dev0)
    dev = tin.device
    n = sa.shape[0]
    o = Opts(sw, max_chain, _EBATCH_FMT[fmt] | flags | (DMX_F_LAZY if lazy else 0), 0)
    if zdict is not None:
        o.flags |= DMX_F_DICT | (DMX_F_FDICT if fdict and fmt == "zlib" else 0)
    # the lengths are known here: the exact block count (a stream outside the tensor has none)
    total = int(tin.numel())
    inside = [(0 <= off <= total and 0 <= ln <= total - off) for off, ln in sa.tolist()]
    good = [int(ln) for (off, ln), ok in zip(sa.tolist(), inside) if ok]
    nblk = encode_batch_blocks(good, sw)
    cap = int((L.dmx_encode_batch_dict_bound if zdict is not None else L.dmx_encode_batch_bound)(sum(good), n, sw, o.flags))
    own = encoder is None
    enc = Encoder(dev.index or 0, 0, sw, max_chain, o.flags) if own else encoder
    # everything runs on one stream: the current one, or a stream of this call's where the current one
    # is the legacy default stream, whose handle 0 would name the encoder's own (unordered) stream
    cur = torch.cuda.current_stream(dev)
    work = cur if cur.cuda_stream else torch.cuda.Stream(dev)
    work.wait_stream(cur)
    try:
        if zdict is None:
            enc.reserve_batch(nblk, n, sw, o.flags)
        else:
            dict_t, dicts_t, nd, of_t = _batch_dicts(zdict, None, dict_of, n, dev)
            enc.reserve_batch_dict(nblk, n, nd, sw, o.flags)
        with torch.cuda.stream(work):
            dt = torch.from_numpy(np.ascontiguousarray(sa)).to(dev) if n else torch.zeros((1, 2), dtype=torch.int64, device=dev)
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            res = torch.zeros(max(n, 1) * 4, dtype=torch.int64, device=dev)
            st = torch.zeros(4, dtype=torch.int64, device=dev)
            if zdict is None:
                _check(compress_batch_async(enc, tin, dt, n, nblk, out, cap, res, st, o), "dmx_encode_batch_async")
            else:
                _check(compress_batch_dict_async(enc, tin, dt, n, nblk, dict_t, dicts_t, nd, of_t, out, cap, res, st, o),
                       "dmx_encode_batch_dict_async")
            offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)   # out_off of every record, then the total
            offsets[:n] = res.view(-1, 4)[:n, 1]
            offsets[n] = st[2]
            host = torch.cat([st, res]).cpu().numpy()   # the call's one synchronisation
        for x in (out, offsets):
            x.record_stream(cur)
        cur.wait_stream(work)
    finally:
        if own:
            enc.close()
    rec = EBatchStatus.from_buffer_copy(host[:4].tobytes())
    results = host[4:4 + 4 * n].view(np.uint8).reshape(-1).view(ERESULT_DTYPE)
    if strict and rec.status:
        raise DeflateError(rec.status, "compress_batch")
    if strict and rec.nfailed:
        raise DeflateError(int(results["status"][rec.first_bad]), f"compress_batch: stream {rec.first_bad}")
    return out[:rec.out_len], offsets, results


def inflate_gpu_chained(z, out_cap: int, index, nblk: int, stream=None, work=None):
    """Inflate on the GPU a stream whose blocks may reference the block before them
    (DMX_F_DICT streams), all blocks in parallel: each decodes into 16-bit cells with
    references for the bytes before it, then pointer jumping resolves the references
    (dmx_inflate_chained_async).  index: Encoder.block_index().  work: optional uint8 CUDA
    scratch of dmx_inflate_chained_work(out_cap, nblk) bytes.  Returns (uint8 tensor, status)."""
    import numpy as np
    import torch
    L = lib()
    dev = z.device
    out = torch.empty(max(out_cap, 1), dtype=torch.uint8, device=dev)
    st = torch.zeros(16, dtype=torch.uint8, device=dev)
    wb = int(L.dmx_inflate_chained_work(out_cap, nblk))
    if work is None or work.numel() < wb:
        work = torch.empty(wb + 256, dtype=torch.uint8, device=dev)
    wp = (work.data_ptr() + 255) & ~255
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    r = L.dmx_inflate_chained_async(z.data_ptr(), z.numel(), index.data_ptr(), nblk, out.data_ptr(), out_cap,
                                    wp, work.numel() - (wp - work.data_ptr()), st.data_ptr(), s)
    _check(r, "dmx_inflate_chained_async")
    torch.cuda.synchronize(dev)
    h = st.cpu().numpy()
    status = int(np.frombuffer(h[:4].tobytes(), np.int32)[0])
    olen = int(np.frombuffer(h[8:16].tobytes(), np.uint64)[0])
    return out[:olen], status


def fault_set(spec: str | None) -> int:
    """Fault injection (tests): "malloc:N" / "launch:N" / None (dmx_fault_set)."""
    return int(lib().dmx_fault_set(spec.encode() if spec else None))


def ref_estimates(tokens, state=None):
    """The reference's estimate fields (tree_bits, ll_bits, d_bits) of every token's
    compress_stats record (deflate_compress.c:290-298), from libdmx's host restatement of its
    adaptive Huffman trees (csrc/dmx_refstats.c).  tokens: uint32 (byte | dist << 9 | len) in
    stream order.  Returns int32[ntok, 3].  Pure host code: no GPU needed."""
    import numpy as np
    t = np.ascontiguousarray(tokens, dtype=np.uint32)
    L = lib()
    e = L.dmx_refest_create() if state is None else state
    rec = np.zeros((t.size, 6), dtype=np.int32)
    nf = ctypes.c_uint32(0)
    try:
        r = L.dmx_refest_feed(e, t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), t.size,
                              ctypes.c_void_p(rec.ctypes.data), ctypes.byref(nf))
    finally:
        if state is None:
            L.dmx_refest_destroy(e)
    _check(r, "dmx_refest_feed")
    return rec[:, 1:4].copy()


def adler32_combine(a: int, b: int, len_b: int) -> int:
    return int(lib().dmx_adler32_combine(a, b, len_b))


def crc32_combine(a: int, b: int, len_b: int) -> int:
    """CRC-32 of A || B from crc(A), crc(B) and len(B) (dmx_crc32_combine; host only)."""
    return int(lib().dmx_crc32_combine(a & 0xFFFFFFFF, b & 0xFFFFFFFF, len_b))


def crc32_geometry() -> tuple[int, int]:
    """(span, lane slice) in bytes of the CRC-32 kernel (dmx_crc32_geometry): a workgroup takes
    a span, each of its lanes a contiguous slice of it."""
    s, l = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib().dmx_crc32_geometry(ctypes.byref(s), ctypes.byref(l))
    return int(s.value), int(l.value)


def gen_text(n: int, seed: int = 0xE5818):
    import numpy as np
    a = np.empty(n, dtype=np.uint8)
    lib().dmx_gen_text(ctypes.c_void_p(a.ctypes.data), n, seed)
    return a


def gen_random(n: int, seed: int = 0x5EED):
    import numpy as np
    a = np.empty(n, dtype=np.uint8)
    lib().dmx_gen_random(ctypes.c_void_p(a.ctypes.data), n, seed)
    return a


class Encoder:
    """Device-resident encoder on one GPU (a dmx_ctx: own HIP stream + HBM workspace).

    encode_async(d_in, n, d_out, cap, stream=None) takes raw device pointers (ints),
    e.g. torch tensors' .data_ptr(); nothing is allocated or synchronised per call.
    """

    def __init__(self, device: int = 0, max_input: int = 1 << 20, sw: int = 32768, max_chain: int = 0,
                 flags: int = DMX_ZLIB):
        self._L = lib()
        self.device = device
        self.opts = Opts(sw, max_chain, flags, 0)
        self._ctx = ctypes.c_void_p()
        _check(self._L.dmx_ctx_create(device, max_input, ctypes.byref(self._ctx)), "dmx_ctx_create")
        if flags & (DMX_F_SPLIT | DMX_F_DICT):   # the block options' scratch (no allocation per encode)
            try:
                self.reserve(max_input, sw, flags)
            except DeflateError:
                self.close()
                raise

    def close(self) -> None:
        if self._ctx:
            self._L.dmx_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, n: int, sw: int = 32768, flags: int = 0) -> None:
        """Workspace for n bytes of sw-byte blocks, plus the scratch of DMX_F_SPLIT / DMX_F_DICT
        (dmx_ctx_reserve_flags; synchronises only when it allocates)."""
        _check(self._L.dmx_ctx_reserve_flags(self._ctx, n, sw, flags), "dmx_ctx_reserve_flags")

    def reserve_batch(self, max_blocks: int, max_streams: int, sw: int = 32768, flags: int = 0) -> None:
        """Workspace for batches (compress_batch_async) of up to max_blocks blocks and max_streams
        streams (dmx_ctx_reserve_batch; synchronises only when it allocates)."""
        _check(self._L.dmx_ctx_reserve_batch(self._ctx, max_blocks, max_streams, sw, flags), "dmx_ctx_reserve_batch")

    def reserve_batch_dict(self, max_blocks: int, max_streams: int, max_dicts: int, sw: int = 32768, flags: int = 0) -> None:
        """Workspace, block table, plan scratch, chain slots for max_blocks + max_dicts and the DICTID
        words of a dictionary batch (dmx_ctx_reserve_batch_dict; synchronises only when it allocates)."""
        _check(self._L.dmx_ctx_reserve_batch_dict(self._ctx, max_blocks, max_streams, max_dicts, sw, flags),
               "dmx_ctx_reserve_batch_dict")

    def encode_async(self, d_in: int, n: int, d_out: int, cap: int, stream: int | None = None,
                     opts: Opts | None = None) -> None:
        o = opts or self.opts
        _check(self._L.dmx_encode_async(self._ctx, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap,
                                        ctypes.byref(o), ctypes.c_void_p(stream or 0)), "dmx_encode_async")

    def result(self, stream: int | None = None) -> Result:
        r = Result()
        _check(self._L.dmx_encode_result(self._ctx, ctypes.byref(r), ctypes.c_void_p(stream or 0)),
               "dmx_encode_result")
        if r.status:
            raise DeflateError(r.status, "encode")
        return r

    def result_async(self, host_ptr: int, stream: int | None = None) -> None:
        """Enqueue the D2H copy of the last encode's 64 B dmx_result into host_ptr (pinned
        memory, e.g. a pin_memory uint8 tensor); read it after the stream or an event."""
        _check(self._L.dmx_encode_result_async(self._ctx, ctypes.c_void_p(host_ptr), ctypes.c_void_p(stream or 0)),
               "dmx_encode_result_async")

    def crc32(self, t, stream=None) -> int:
        """CRC-32 (RFC 1952 / PNG) of a uint8 CUDA tensor, computed on the device
        (dmx_crc32_async); the tensor's storage may start at any byte."""
        import torch
        n = t.numel()
        self.reserve(n, 32768)
        w = torch.empty(1, dtype=torch.int32, device=t.device)
        s = stream if stream is not None else torch.cuda.current_stream(t.device).cuda_stream
        if not s:   # the default stream's handle is NULL, which selects the context's own stream
            torch.cuda.synchronize(t.device)
        _check(self._L.dmx_crc32_async(self._ctx, ctypes.c_void_p(t.data_ptr() if n else 0), n,
                                       ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(s)), "dmx_crc32_async")
        torch.cuda.synchronize(t.device)
        return int(w.item()) & 0xFFFFFFFF

    def crc32_blocks(self, t, sw: int = 32768, stream=None):
        """CRC-32 of every sw-byte block of a uint8 CUDA tensor (the last one may be short),
        computed on the device (dmx_crc32_blocks_async): an int32 CUDA tensor of ceil(n / sw)
        words (view as uint32 on the host).  The tensor's storage may start at any byte."""
        import torch
        n = t.numel()
        nb = (n + sw - 1) // sw
        w = torch.empty(max(nb, 1), dtype=torch.int32, device=t.device)
        s = stream if stream is not None else torch.cuda.current_stream(t.device).cuda_stream
        if not s:   # the default stream's handle is NULL, which selects the context's own stream
            torch.cuda.synchronize(t.device)
        _check(self._L.dmx_crc32_blocks_async(self._ctx, ctypes.c_void_p(t.data_ptr() if n else 0), n, sw,
                                              ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(s)), "dmx_crc32_blocks_async")
        torch.cuda.synchronize(t.device)
        return w[:nb]

    # -- introspection of the last encode (tests / stats) --
    def blocks(self, nblk: int):
        import numpy as np
        nt = np.zeros(nblk, np.uint32)
        bt = np.zeros(nblk, np.uint8)
        hb = np.zeros(nblk, np.uint32)
        r = self._L.dmx_last_blocks(self._ctx, nt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                    bt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                    hb.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), nblk)
        if r < 0:
            raise DeflateError(r, "dmx_last_blocks")
        return nt[:r], bt[:r], hb[:r]

    def tokens(self, blk: int):
        import numpy as np
        t = np.zeros(32768, np.uint32)
        r = self._L.dmx_last_tokens(self._ctx, blk, t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 32768)
        if r < 0:
            raise DeflateError(r, "dmx_last_tokens")
        return t[:r].copy()

    def code_lengths(self, blk: int):
        import numpy as np
        ln = np.zeros(316, np.uint8)
        _check(self._L.dmx_last_code_lengths(self._ctx, blk, ln.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
               "dmx_last_code_lengths")
        return ln

    def subblocks(self, blk: int):
        """DEFLATE blocks of sw block `blk` in the last encode (f3 split: up to 4):
        list of (t0, t1, btype, hdr_bits, code lengths[316])."""
        import numpy as np
        out = []
        nsub, k = 1, 0
        while k < nsub:
            rg = np.zeros(2, np.uint32)
            bt = np.zeros(1, np.uint32)
            hb = np.zeros(1, np.uint32)
            ln = np.zeros(316, np.uint8)
            P = ctypes.POINTER(ctypes.c_uint32)
            nsub = self._L.dmx_last_subblock(self._ctx, blk, k, rg.ctypes.data_as(P), bt.ctypes.data_as(P),
                                             hb.ctypes.data_as(P), ln.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
            if nsub < 0:
                raise DeflateError(nsub, "dmx_last_subblock")
            out.append((int(rg[0]), int(rg[1]), int(bt[0]), int(hb[0]), ln))
            k += 1
        return out

    def stamps(self, nblk: int):
        """[nblk, 16] match-kernel phase cycles (needs DMX_STAMPS=1): P0, search, walk+compaction,
        deferred extension, search steps, W1, W1-W3, total, then P0 sub-phase ends (staged,
        pass 1, pass 2) relative to the kernel start."""
        import numpy as np
        a = np.zeros((nblk, 16), np.uint64)
        _check(self._L.dmx_debug_stamps(self._ctx, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), nblk),
               "dmx_debug_stamps")
        return a

    def block_index(self, stream=None):
        """Device block index of the last encode (uint8 tensor of nblk x 24 B dmx_iblock
        records) for inflate_gpu's parallel mode."""
        import torch
        n = self.last_nblk()
        ix = torch.empty(max(n, 1) * 24, dtype=torch.uint8, device=f"cuda:{self.device}")
        s = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        r = self._L.dmx_block_index(self._ctx, ix.data_ptr(), n, s)
        if r < 0:
            raise DeflateError(r, "dmx_block_index")
        return ix, n

    def last_nblk(self) -> int:
        return int(self._L.dmx_last_blocks(self._ctx, None, None, None, 1 << 30))

    STAGES = ("pre", "match", "huff", "scan", "pack")

    HOOKS = {"worklist": 1, "dedupe": 2, "scan3": 3, "bdict_simple": 4}   # DMX_HOOK_* (include/dmx.h)
    WORKLIST = {None: -1, "0": 0, "list": 1, "plain": 2}

    def set_hook(self, name: str, value) -> None:
        """Test hooks of this context (dmx_ctx_set_hook): "worklist" None (adaptive) / "0" /
        "list" / "plain"; "dedupe" None / 0 / 1; "scan3" 0 / 1; "bdict_simple" 0 / 1.  Every setting must give the
        same stream; they pick launch shapes only."""
        if name == "worklist":
            v = self.WORKLIST[value]
        elif name == "dedupe":
            v = -1 if value is None else int(value)
        else:
            v = int(value)
        _check(self._L.dmx_ctx_set_hook(self._ctx, self.HOOKS[name], v), "dmx_ctx_set_hook")

    def set_timing(self, on: bool, stage: str | None = None, every: int = 1) -> None:
        """HIP-event stage times of the following encodes: every stage boundary, or with
        `stage` only that stage's two events (a timed loop then pays two event records per
        encode; the other stages read 0), on every `every`-th encode (1..255)."""
        if not 1 <= every <= 255:
            raise ValueError("every must be 1..255")
        mode = 0 if not on else (1 if stage is None else 0x100 | self.STAGES.index(stage) | (every << 12))
        self._L.dmx_ctx_set_timing(self._ctx, mode)

    def stage_times(self):
        ms = (ctypes.c_double * 6)()
        cnt = ctypes.c_uint32(0)
        self._L.dmx_ctx_stage_times(self._ctx, ms, ctypes.byref(cnt))
        return {k: v for k, v in zip(["pre", "match", "huff", "scan", "pack", "total"], list(ms))}, cnt.value

    # -- host convenience on this context via torch tensors --
    def compress_tensor(self, t_in, stream=None, opts: Opts | None = None):
        """Encode a uint8 CUDA tensor; returns (uint8 CUDA tensor of the stream, Result)."""
        import torch
        o = opts or self.opts
        n = t_in.numel()
        self.reserve(n, o.sw, o.flags)
        cap = max_compressed(n, o.sw, o.flags)
        out = torch.empty(cap, dtype=torch.uint8, device=t_in.device)
        s = stream if stream is not None else torch.cuda.current_stream(t_in.device).cuda_stream
        self.encode_async(t_in.data_ptr() if n else out.data_ptr(), n, out.data_ptr(), cap, s, o)
        r = self.result(s)
        return out[:r.out_len], r

    def compress_bytes(self, data, sw: int = 32768, max_chain: int = 0, flags: int = DMX_ZLIB, pre=None):
        """Host bytes -> HBM -> encode -> host bytes, on this context (keeps introspection).
        pre: DMX_F_DICT history of block 0 (host bytes, staged in HBM here); with DMX_F_FDICT in flags
        the zlib header names it (1 <= len(pre) <= sw)."""
        import numpy as np
        import torch
        dev = f"cuda:{self.device}"
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        t = torch.from_numpy(a.copy()).to(dev) if a.size else torch.empty(0, dtype=torch.uint8, device=dev)
        self.reserve(a.size, sw, flags)
        o = Opts(sw, max_chain, flags, 0)
        if pre is not None and len(pre):
            tp = torch.from_numpy(np.frombuffer(bytes(pre), dtype=np.uint8).copy()).to(dev)
            o.dict, o.dict_len = tp.data_ptr(), tp.numel()
        out, r = self.compress_tensor(t, opts=o)
        return out.cpu().numpy().tobytes(), r
