"""The dictionary batch encode without a device: the exports and their declarations, every argument
error that dmx_encode_batch_dict_async and dmx_ctx_reserve_batch_dict return before any device call
(a zeroed block of memory stands in for a context that was never reserved, as in
test_compress_batch_api.py), dmx_encode_batch_dict_bound (monotone; at least the sum of the single
encodes' bounds on random partitions), and the host twin of the plan
(tests/c/encode_batch_dict_model.cpp: the dmx_ebd_* text of csrc/dmx_encode_batch.h as loops against
brute force under ASan + UBSan, stand-alone programs)."""
import ctypes
import os
import random
import subprocess

import pytest

import deflate_compression_amd as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE, SZ = -E["E_INVAL"], -E["E_RANGE"], -E["E_SZ"]
vp = ctypes.c_void_p
DICT, FD = D.DMX_F_DICT, D.DMX_F_FDICT
FRAMINGS = (D.DMX_ZLIB | DICT, D.DMX_ZLIB | DICT | FD, D.DMX_F_FINAL | DICT)


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in ("dmx_encode_batch_dict_bound", "dmx_encode_batch_dict_geometry", "dmx_ctx_reserve_batch_dict",
                 "dmx_encode_batch_dict_async"):
        f = getattr(L, name)
        assert f.argtypes is not None, name
        assert name + "(" in hdr, name
    assert "#define DMX_HOOK_BDICT_SIMPLE 4" in hdr
    for name in ("compress_batch", "compress_batch_dict_async", "BDict", "DMX_BATCH_NODICT"):
        assert name in D.__all__ and hasattr(D, name), name
    assert hasattr(D.Encoder, "reserve_batch_dict") and D.Encoder.HOOKS["bdict_simple"] == 4
    blob = open(D.LIB_PATH, "rb").read()
    for k in (b"dmx_eb_table_kernel", b"dmx_ebd_chain_kernel", b"dmx_ebd_hist_kernel", b"dmx_ebd_match_kernel",
              b"dmx_ebd_store_check_kernel", b"dmx_eb_scan_apply1_kernel", b"dmx_ebd_finish_kernel"):
        assert k in blob, k


def test_python_argument_errors():
    # refused before anything touches a device
    with pytest.raises(ValueError):
        D.compress_batch([b"abc"], fmt="gzip", zdict=b"abc")
    with pytest.raises(ValueError):
        D.compress_batch([b"abc"], dict_of=[0])


_FAKE_CTX = ctypes.create_string_buffer(1 << 16)


def _call(ctx=None, d_in=0x1000, in_bytes=64, streams=0x2000, n=3, max_blocks=3, d_dict=0x6000, dict_bytes=32, dicts=0x7000,
          ndicts=1, dict_of=0x8000, opts=None, null_opts=False, out=0x3000, out_cap=64, results=0x4000, status=0x5000):
    """dmx_encode_batch_dict_async on made-up addresses: an argument error returns before they are used"""
    L = D.lib()
    if ctx is None:
        ctx = ctypes.addressof(_FAKE_CTX)
    o = opts or D.Opts(1024, 7, D.DMX_ZLIB | DICT | FD, 0)
    return L.dmx_encode_batch_dict_async(vp(ctx), vp(d_in), in_bytes, vp(streams), n, max_blocks, vp(d_dict), dict_bytes,
                                         vp(dicts), ndicts, vp(dict_of), None if null_opts else ctypes.byref(o), vp(out),
                                         out_cap, vp(results), vp(status), vp(0))


def test_argument_errors():
    assert _call(ctx=0) == INVAL
    assert _call(out=0) == INVAL
    assert _call(results=0) == INVAL
    assert _call(status=0) == INVAL
    assert _call(d_in=0) == INVAL                        # NULL with in_bytes > 0
    assert _call(streams=0) == INVAL                     # NULL with nstreams > 0
    assert _call(dicts=0) == INVAL                       # NULL with ndicts > 0
    assert _call(d_dict=0) == INVAL                      # NULL with dict_bytes > 0
    assert _call(streams=0x2004) == INVAL                # 8-byte alignment of the descriptors
    assert _call(results=0x4004) == INVAL
    assert _call(status=0x5004) == INVAL
    assert _call(dicts=0x7004) == INVAL                  # ... of the dictionary records
    assert _call(dict_of=0x8002) == INVAL                # 4-byte alignment of the indices
    assert _call(out=0x3002) == INVAL                    # ... and of the output
    Z, F, H, T = D.DMX_ZLIB, D.DMX_F_FINAL, D.DMX_F_HEADER, D.DMX_F_TRAILER
    for fl in (Z, F, Z | FD,                                          # no DMX_F_DICT
               DICT, H | T | DICT,                                    # no DMX_F_FINAL
               F | H | DICT, F | T | DICT,                            # half a container
               F | DICT | FD, F | T | DICT | FD,                      # DMX_F_FDICT without a zlib header
               D.DMX_GZIP | DICT, D.DMX_GZIP | DICT | FD, F | D.DMX_F_GZIP | DICT,
               D.DMX_BGZF | DICT, Z | D.DMX_F_BGZF | DICT, Z | D.DMX_F_SPLIT | DICT, Z | D.DMX_F_SPLIT | DICT | FD):
        assert _call(opts=D.Opts(1024, 7, fl, 0)) == INVAL, fl
    assert _call(null_opts=True) == INVAL                # NULL opts are a plain zlib stream: no DMX_F_DICT
    for fr in FRAMINGS:
        for o in (D.Opts(-1, 7, fr, 0), D.Opts(32769, 7, fr, 0), D.Opts(1024, -1, fr, 0), D.Opts(1024, 7, fr, -1),
                  D.Opts(1024, 7, fr, 256)):
            assert _call(opts=o) == RANGE
    assert _call(n=0x80000000) == RANGE
    assert _call(max_blocks=0x80000000) == RANGE
    assert _call(ndicts=0x80000000) == RANGE
    # a NULL beats a bad flag, a bad flag a bad range
    assert _call(status=0, opts=D.Opts(1024, 7, 0, 0)) == INVAL
    assert _call(opts=D.Opts(-1, 7, D.DMX_ZLIB, 0)) == INVAL
    # every allowed framing and parse / block option passes the checks: what is left is the reservation
    for fr in FRAMINGS:
        for extra in (0, D.DMX_F_LAZY, D.DMX_F_DEEP, D.DMX_F_STORE_CHECK, D.DMX_F_EXACT_SORT,
                      D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK):
            for sw in (0, 1, 64, 32768):
                assert _call(opts=D.Opts(sw, 0, fr | extra, 0)) == SZ
    assert _call(dict_of=0) == SZ                        # NULL d_dict_of: every stream uses dictionary 0
    assert _call(ndicts=0, dicts=0, d_dict=0, dict_bytes=0, dict_of=0) == SZ
    assert _call(n=0, max_blocks=0, streams=0, d_in=0, in_bytes=0) == SZ   # even the empty batch needs the reservation


def test_reserve_argument_errors():
    L = D.lib()
    ctx = ctypes.addressof(_FAKE_CTX)
    assert L.dmx_ctx_reserve_batch_dict(vp(0), 1, 1, 1, 1024, 0) == INVAL
    assert L.dmx_ctx_reserve_batch_dict(vp(ctx), 1, 1, 1, -1, 0) == RANGE
    assert L.dmx_ctx_reserve_batch_dict(vp(ctx), 1, 1, 1, 32769, 0) == RANGE
    assert L.dmx_ctx_reserve_batch_dict(vp(ctx), 0x80000000, 1, 1, 1024, 0) == RANGE
    assert L.dmx_ctx_reserve_batch_dict(vp(ctx), 1, 0x80000000, 1, 1024, 0) == RANGE
    assert L.dmx_ctx_reserve_batch_dict(vp(ctx), 1, 1, 0x80000000, 1024, 0) == RANGE
    for fl in (D.DMX_F_GZIP, D.DMX_F_SPLIT, D.DMX_F_BGZF):
        assert L.dmx_ctx_reserve_batch_dict(vp(ctx), 1, 1, 1, 1024, fl) == INVAL
    # the old reservation still refuses the dictionary flags
    for fl in (DICT, FD):
        assert L.dmx_ctx_reserve_batch(vp(ctx), 1, 1, 1024, fl) == INVAL
    assert L.dmx_ctx_set_hook(vp(ctx), 4, 2) == RANGE and L.dmx_ctx_set_hook(vp(ctx), 4, -1) == RANGE


def _partition(rng, total, n):
    if n == 0:
        return []
    cuts = sorted(rng.randint(0, total) for _ in range(n - 1))
    if rng.random() < 0.5:
        cuts = sorted(c if rng.random() < 0.7 else cuts[0] for c in cuts)
    edges = [0] + cuts + [total]
    return [b - a for a, b in zip(edges, edges[1:])]


def test_bound():
    L = D.lib()
    rng = random.Random(21)
    for sw in (0, 1, 7, 64, 1024, 32768):
        for flags in FRAMINGS:
            last = 0
            for total in (0, 1, 63, 64, 65, 4096, 100000, 1 << 20, 1 << 33):
                c = L.dmx_encode_batch_dict_bound(total, 5, sw, flags)
                assert c >= last and c % 4 == 0                           # monotone in total_in
                last = c
            last = 0
            for n in (0, 1, 2, 3, 100, 1 << 16, 0x7FFFFFFF):
                c = L.dmx_encode_batch_dict_bound(100000, n, sw, flags)
                assert c >= last                                          # ... and in nstreams
                last = c
            # 4 more per stream under DMX_F_FDICT, the plain batch's bound otherwise
            plain = L.dmx_encode_batch_bound(100000, 100, sw, flags & ~(DICT | FD))
            assert L.dmx_encode_batch_dict_bound(100000, 100, sw, flags) == plain + (400 if flags & FD else 0)
    assert L.dmx_encode_batch_dict_bound(2 ** 64 - 1, 0xFFFFFFFF, 1, D.DMX_ZLIB | DICT | FD) >= 2 ** 64 - 4   # saturates
    for it in range(300):
        sw = rng.choice((1, 3, 64, 1000, 1024, 32768))
        n = rng.choice((0, 1, 2, 5, 17, 100))
        total = 0 if n == 0 else rng.choice((0, 1, sw - 1, sw, sw + 1, 10 * sw, rng.randint(0, 300000)))
        lens = _partition(rng, total, n)
        assert sum(lens) == total and len(lens) == n
        for flags in FRAMINGS:
            need = sum((L.dmx_max_compressed_flags(x, sw, flags) + 3) & ~3 for x in lens)
            assert L.dmx_encode_batch_dict_bound(total, n, sw, flags) >= need, (total, n, sw, flags)


def test_host_twin_asan_ubsan():
    """tests/c/encode_batch_dict_model.cpp ends with `0 failed checks`, with scan tiles of 4 and of 8
    streams: bad buffers, bad dictionary indices, records outside d_dict (off + len wrapping 2^64
    included), lengths 0 and sw + 1 under both settings of DMX_F_FDICT, DMX_BATCH_NODICT, a NULL
    d_dict_of and ndicts 0, at capacities below, at and above the need."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.encode_batch_dict"])
    for exe in ("encode_batch_dict_model4", "encode_batch_dict_model8"):
        p = subprocess.run([os.path.join(REPO, "build", "c", exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert " checks, 0 failed checks" in p.stdout
