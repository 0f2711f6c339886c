"""The batch encode without a device: the exports and their declarations, the three structs, the
argument errors that dmx_encode_batch_async and dmx_ctx_reserve_batch return before any device
call, the two bounds (monotone; at least the real block count and the sum of the single encodes'
bounds on random partitions), and the host twin of the plan (tests/c/encode_batch_model.cpp:
csrc/dmx_encode_batch.h as loops against brute force under ASan + UBSan, stand-alone programs)."""
import ctypes
import os
import random
import subprocess

import deflate_compression_amd as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE, SZ = -E["E_INVAL"], -E["E_RANGE"], -E["E_SZ"]
vp = ctypes.c_void_p
FRAMINGS = (D.DMX_ZLIB, D.DMX_GZIP, D.DMX_F_FINAL)


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in ("dmx_encode_batch_blocks", "dmx_encode_batch_bound", "dmx_ctx_reserve_batch", "dmx_encode_batch_async"):
        f = getattr(L, name)
        assert f.argtypes is not None, name
        assert name + "(" in hdr, name
    for name in ("dmx_estream", "dmx_eresult", "dmx_ebatch_status", "78 9C 03 00 00 00 00 01"):
        assert name in hdr, name
    for name in ("compress_batch", "compress_batch_async", "encode_batch_blocks", "EStream", "EResult", "EBatchStatus",
                 "ERESULT_DTYPE"):
        assert name in D.__all__ and hasattr(D, name), name
    blob = open(D.LIB_PATH, "rb").read()
    for k in (b"dmx_eb_table_kernel", b"dmx_eb_match_kernel", b"dmx_eb_scan_apply1_kernel", b"dmx_eb_pack_kernel",
              b"dmx_eb_finish_kernel", b"dmx_eb_crc_kernel"):
        assert k in blob, k


def test_struct_sizes():
    import numpy as np
    assert ctypes.sizeof(D.EStream) == 16
    assert ctypes.sizeof(D.EResult) == 32
    assert ctypes.sizeof(D.EBatchStatus) == 32
    assert [getattr(D.EStream, f).offset for f, _ in D.EStream._fields_] == [0, 8]
    assert [getattr(D.EResult, f).offset for f, _ in D.EResult._fields_] == [0, 4, 8, 16, 24, 28]
    assert [getattr(D.EBatchStatus, f).offset for f, _ in D.EBatchStatus._fields_] == [0, 4, 8, 12, 16, 24]
    dt = np.dtype(D.ERESULT_DTYPE)
    assert dt.itemsize == 32 and [dt.fields[f][1] for f, _ in D.EResult._fields_] == [0, 4, 8, 16, 24, 28]


# a context that was never reserved for a batch: zeroed memory in place of a dmx_ctx (every argument
# error returns before the context is used; the reservation check reads its capacities, all 0)
_FAKE_CTX = ctypes.create_string_buffer(1 << 16)


def _call(ctx=None, d_in=0x1000, in_bytes=64, streams=0x2000, n=3, max_blocks=3, opts=None, null_opts=False, out=0x3000,
          out_cap=64, results=0x4000, status=0x5000):
    """dmx_encode_batch_async on made-up addresses: an argument error returns before they are used"""
    L = D.lib()
    if ctx is None:
        ctx = ctypes.addressof(_FAKE_CTX)
    o = opts or D.Opts(1024, 7, D.DMX_ZLIB, 0)
    return L.dmx_encode_batch_async(vp(ctx), vp(d_in), in_bytes, vp(streams), n, max_blocks, None if null_opts else ctypes.byref(o),
                                    vp(out), out_cap, vp(results), vp(status), vp(0))


def test_argument_errors():
    assert _call(ctx=0) == INVAL
    assert _call(out=0) == INVAL
    assert _call(results=0) == INVAL
    assert _call(status=0) == INVAL
    assert _call(d_in=0) == INVAL                        # NULL with in_bytes > 0
    assert _call(streams=0) == INVAL                     # NULL with nstreams > 0
    assert _call(streams=0x2004) == INVAL                # 8-byte alignment of the descriptors
    assert _call(results=0x4004) == INVAL                # ... of the results
    assert _call(status=0x5004) == INVAL                 # ... of the record
    assert _call(out=0x3002) == INVAL                    # 4-byte alignment of the output
    # the framing must make a complete stream
    for fl in (0, D.DMX_F_HEADER, D.DMX_F_TRAILER, D.DMX_F_HEADER | D.DMX_F_TRAILER,       # no DMX_F_FINAL
               D.DMX_F_FINAL | D.DMX_F_HEADER, D.DMX_F_FINAL | D.DMX_F_TRAILER,             # half a container
               D.DMX_F_FINAL | D.DMX_F_GZIP | D.DMX_F_TRAILER, D.DMX_F_FINAL | D.DMX_F_GZIP,
               D.DMX_ZLIB | D.DMX_F_DICT, D.DMX_ZLIB | D.DMX_F_SPLIT, D.DMX_BGZF, D.DMX_ZLIB | D.DMX_F_BGZF,
               D.DMX_GZIP | D.DMX_F_SPLIT):
        assert _call(opts=D.Opts(1024, 7, fl, 0)) == INVAL, fl
    # sw, max_chain, deep_chain as dmx_encode_async checks them
    for o in (D.Opts(-1, 7, D.DMX_ZLIB, 0), D.Opts(32769, 7, D.DMX_ZLIB, 0), D.Opts(1024, -1, D.DMX_ZLIB, 0),
              D.Opts(1024, 7, D.DMX_ZLIB, -1), D.Opts(1024, 7, D.DMX_ZLIB, 256)):
        assert _call(opts=o) == RANGE
    assert _call(n=0x80000000) == RANGE
    assert _call(max_blocks=0x80000000) == RANGE
    # a NULL beats a bad flag, a bad flag a bad range
    assert _call(status=0, opts=D.Opts(1024, 7, 0, 0)) == INVAL
    assert _call(opts=D.Opts(-1, 7, 0, 0)) == INVAL
    # every framing and every parse / block option passes the checks: what is left is the reservation
    for fr in FRAMINGS:
        for extra in (0, D.DMX_F_LAZY, D.DMX_F_DEEP, D.DMX_F_STORE_CHECK, D.DMX_F_EXACT_SORT,
                      D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK):
            for sw in (0, 1, 64, 32768):
                assert _call(opts=D.Opts(sw, 0, fr | extra, 0)) == SZ
    assert _call(null_opts=True) == SZ                   # NULL opts: a zlib stream, exhaustive, sw 32768
    assert _call(n=0, max_blocks=0, streams=0, d_in=0, in_bytes=0) == SZ   # even the empty batch needs the plan's scratch


def test_reserve_argument_errors():
    L = D.lib()
    ctx = ctypes.addressof(_FAKE_CTX)
    assert L.dmx_ctx_reserve_batch(vp(0), 1, 1, 1024, 0) == INVAL
    assert L.dmx_ctx_reserve_batch(vp(ctx), 1, 1, -1, 0) == RANGE
    assert L.dmx_ctx_reserve_batch(vp(ctx), 1, 1, 32769, 0) == RANGE
    assert L.dmx_ctx_reserve_batch(vp(ctx), 0x80000000, 1, 1024, 0) == RANGE
    assert L.dmx_ctx_reserve_batch(vp(ctx), 1, 0x80000000, 1024, 0) == RANGE
    for fl in (D.DMX_F_DICT, D.DMX_F_SPLIT, D.DMX_F_BGZF):
        assert L.dmx_ctx_reserve_batch(vp(ctx), 1, 1, 1024, fl) == INVAL


def _partition(rng, total, n):
    """total split into n lengths, empty ones included"""
    if n == 0:
        return []
    cuts = sorted(rng.randint(0, total) for _ in range(n - 1))
    if rng.random() < 0.5:   # some equal cuts: empty streams
        cuts = sorted(c if rng.random() < 0.7 else cuts[0] for c in cuts)
    edges = [0] + cuts + [total]
    return [b - a for a, b in zip(edges, edges[1:])]


def test_bounds():
    L = D.lib()
    rng = random.Random(20)
    for sw in (0, 1, 7, 64, 1024, 32768):
        for flags in FRAMINGS:
            lastb, lastc = 0, 0
            for total in (0, 1, 63, 64, 65, 4096, 100000, 1 << 20, 1 << 33):
                b, c = L.dmx_encode_batch_blocks(total, 5, sw), L.dmx_encode_batch_bound(total, 5, sw, flags)
                assert b >= lastb and c >= lastc and c % 4 == 0          # monotone in total_in
                lastb, lastc = b, c
            lastb, lastc = 0, 0
            for n in (0, 1, 2, 3, 100, 1 << 16, 0x7FFFFFFF):
                b, c = L.dmx_encode_batch_blocks(100000, n, sw), L.dmx_encode_batch_bound(100000, n, sw, flags)
                assert b >= lastb and c >= lastc                          # ... and in nstreams
                lastb, lastc = b, c
    assert L.dmx_encode_batch_blocks(2 ** 64 - 1, 0xFFFFFFFF, 1) == 0xFFFFFFFF   # saturate
    assert L.dmx_encode_batch_bound(2 ** 64 - 1, 0xFFFFFFFF, 1, D.DMX_GZIP) >= 2 ** 64 - 4
    for it in range(300):
        sw = rng.choice((1, 3, 64, 1000, 1024, 32768))
        n = rng.choice((0, 1, 2, 5, 17, 100))
        total = 0 if n == 0 else rng.choice((0, 1, sw - 1, sw, sw + 1, 10 * sw, rng.randint(0, 300000)))
        lens = _partition(rng, total, n)
        assert sum(lens) == total and len(lens) == n
        real = D.encode_batch_blocks(lens, sw)
        assert real == sum(max(1, (x + sw - 1) // sw) for x in lens)
        assert L.dmx_encode_batch_blocks(total, n, sw) >= real, (total, n, sw)
        for flags in FRAMINGS:
            need = sum((L.dmx_max_compressed_flags(x, sw, flags) + 3) & ~3 for x in lens)
            assert L.dmx_encode_batch_bound(total, n, sw, flags) >= need, (total, n, sw, flags)


def test_host_twin_asan_ubsan():
    """tests/c/encode_batch_model.cpp ends with `0 failed checks`, with scan tiles of 4 and of 8
    streams: for fixed lists with the lengths 0, 1, sw - 1, sw, sw + 1, offsets at the end of the input
    and in_off + in_len wrapping 2^64, and for 1 500 seeded random lists, at capacities below, at and
    above the need, the plan's block table, starts, records and its -E_RANGE / -E_SZ decisions are
    those of a brute-force loop."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.encode_batch"])
    for exe in ("encode_batch_model4", "encode_batch_model8"):
        p = subprocess.run([os.path.join(REPO, "build", "c", exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert " checks, 0 failed checks" in p.stdout
