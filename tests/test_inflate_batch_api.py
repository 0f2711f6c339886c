"""The batch inflate without a device: the exports and their declarations, the three structs, the
argument errors that dmx_inflate_batch_async returns before any device call, the size of the work
buffer, and the host twin of the framing the kernel runs per stream (tests/c/gz_head_model.cpp:
csrc/dmx_gz_head.h against deflate_decompress under ASan + UBSan, a stand-alone program)."""
import ctypes
import os
import subprocess

import deflate_compression_amd as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE = -E["E_INVAL"], -E["E_RANGE"]
vp = ctypes.c_void_p


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in ("dmx_inflate_batch_work", "dmx_inflate_batch_async"):
        f = getattr(L, name)
        assert f.argtypes is not None, name
        assert name + "(" in hdr, name
    for name in ("dmx_bstream", "dmx_bresult", "dmx_batch_status", "DMX_BATCH_AUTO 0u", "DMX_BATCH_ZLIB 1u",
                 "DMX_BATCH_GZIP 2u", "DMX_BATCH_RAW  3u", "DMX_BATCH_MEASURE 16u", "a wrong CRC-32 passes"):
        assert name in hdr, name
    for name in ("inflate_batch", "inflate_batch_async", "BStream", "BResult", "BatchStatus", "DMX_BATCH_AUTO",
                 "DMX_BATCH_ZLIB", "DMX_BATCH_GZIP", "DMX_BATCH_RAW", "DMX_BATCH_MEASURE"):
        assert name in D.__all__ and hasattr(D, name), name
    assert (D.DMX_BATCH_AUTO, D.DMX_BATCH_ZLIB, D.DMX_BATCH_GZIP, D.DMX_BATCH_RAW, D.DMX_BATCH_MEASURE) == (0, 1, 2, 3, 16)


def test_struct_sizes():
    import numpy as np
    assert ctypes.sizeof(D.BStream) == 32
    assert ctypes.sizeof(D.BResult) == 32
    assert ctypes.sizeof(D.BatchStatus) == 16
    assert [getattr(D.BStream, f).offset for f, _ in D.BStream._fields_] == [0, 8, 16, 24]
    assert [getattr(D.BResult, f).offset for f, _ in D.BResult._fields_] == [0, 4, 8, 16, 24, 28]
    assert [getattr(D.BatchStatus, f).offset for f, _ in D.BatchStatus._fields_] == [0, 4, 8]
    dt = np.dtype(D.BRESULT_DTYPE)
    assert dt.itemsize == 32 and [dt.fields[f][1] for f, _ in D.BResult._fields_] == [0, 4, 8, 16, 24, 28]


def _call(z=0x1000, zbytes=64, streams=0x2000, n=3, flags=0, out=0x3000, out_bytes=64, results=0x4000, work=0x10000,
          work_bytes=None, status=0x5000):
    """dmx_inflate_batch_async on made-up addresses: an argument error returns before they are used"""
    L = D.lib()
    if work_bytes is None:
        work_bytes = L.dmx_inflate_batch_work(n)
    return L.dmx_inflate_batch_async(vp(z), zbytes, vp(streams), n, flags, vp(out), out_bytes, vp(results), vp(work),
                                     work_bytes, vp(status), vp(0))


def test_argument_errors():
    L = D.lib()
    need = L.dmx_inflate_batch_work(3)
    assert _call(results=0) == INVAL
    assert _call(status=0) == INVAL
    assert _call(work=0) == INVAL
    assert _call(streams=0) == INVAL                    # NULL with nstreams > 0
    assert _call(z=0) == INVAL                          # NULL with zbytes > 0
    assert _call(out=0) == INVAL                        # NULL without the measure flag
    for fmt in (0, 1, 2, 3):
        assert _call(out=0, flags=fmt) == INVAL
    assert _call(streams=0x2004) == INVAL               # 8-byte alignment of the descriptors
    assert _call(results=0x4004) == INVAL               # ... of the results
    assert _call(status=0x5004) == INVAL                # ... of the record
    assert _call(work=0x10080) == INVAL                 # 256-byte alignment of the work buffer
    assert _call(work_bytes=need - 1) == INVAL
    assert _call(work_bytes=0) == INVAL
    for flags in (4, 15, 32, 3 | 32, 16 | 7, 0x80000000, 0x100):
        assert _call(flags=flags) == RANGE, flags
    # the argument checks come first, in the order of the contract: a NULL beats a bad flag
    assert _call(status=0, flags=32) == INVAL


def test_work_size():
    L = D.lib()
    last = 0
    for n in (0, 1, 2, 3, 63, 64, 255, 256, 1023, 1024, 1025, 2047, 2048, 4096, 1 << 20, 0x7FFFFFFF, 0xFFFFFFFF):
        w = L.dmx_inflate_batch_work(n)
        assert w >= 256 and w % 256 == 0 and w >= last, (n, w)
        last = w
    # a table area of 8 KiB per workgroup, and a bound on the workgroups: the buffer stops growing
    assert L.dmx_inflate_batch_work(2) - L.dmx_inflate_batch_work(1) == 8192
    assert L.dmx_inflate_batch_work(0xFFFFFFFF) == L.dmx_inflate_batch_work(1 << 20) <= 64 << 20


def test_host_twin_asan_ubsan():
    """tests/c/gz_head_model.cpp ends with `0 failed checks`: for all 16 combinations of the optional
    gzip header fields in three sizes, every cut point, the reserved bits, every CM and zlib CMF, and
    10 000 seeded mutations, the verdict of the framing text the kernel runs is deflate_decompress's
    status, and where it is 0 the host decodes the same bytes from the offset it names."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.gz_head"])
    exe = os.path.join(REPO, "build", "c", "gz_head_model")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert " checks, 0 failed checks" in p.stdout
