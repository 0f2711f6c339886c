"""The seek-point index from the one-pass decode, without a GPU (dmx_zindex_from_parallel_async's
checks before any device call, dmx_zindex_points_bound, dmx_zindex_device_work, and the host twin
dmx_zindex_from_chunks_host): the exports and their declarations, the argument errors from made-up
addresses, the size functions, the host twin on the host plan's chunks and zlib's output pinned to
zlib's own verdict on every point (check_index and check_points of test_zindex_api.py), and the
selection rule under the sanitizers (tests/c/zsel_model.cpp: ASan + UBSan, a stand-alone program)."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import deflate_compression_amd as D
import inflate_parallel_inputs as I
import test_zindex_api as ZA
import zindex_gpu_inputs as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE = -E["E_INVAL"], -E["E_RANGE"]
vp = ctypes.c_void_p
CALLS = ("dmx_zindex_points_bound", "dmx_zindex_device_work", "dmx_zindex_from_parallel_async", "dmx_zindex_from_chunks_host")
W = 32768


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in CALLS:
        f = getattr(L, name)
        assert f.argtypes is not None, name
        assert name + "(" in hdr, name
        decl = re.search(r"^\w+\s+" + name + r"\(([^;]*?)\);", hdr, re.S | re.M).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(f.argtypes) == len([a for a in decl.split(",") if a.strip() not in ("", "void")]), name
    assert "Seek points from the one-pass decode" in hdr
    for name in ("zindex_from_parallel_async", "inflate_parallel_indexed"):
        assert name in D.__all__ and callable(getattr(D, name)), name
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "inflate_parallel_indexed" in open(os.path.join(REPO, doc)).read(), doc
    assert os.path.exists(os.path.join(REPO, "deflate_compression_amd", "csrc", "dmx_zsel.h"))


def _call(plan=0x10000, plan_bytes=None, dec=0x5000, out=0x3000, out_cap=4096, max_live=8, span=0, points=0x2000, adlers=0x6000,
          windows=0x80000, max_points=3, work=0x20000, work_bytes=None, status=0x7000):
    """dmx_zindex_from_parallel_async on made-up addresses: an argument error returns before they are used"""
    L = D.lib()
    if plan_bytes is None:
        plan_bytes = L.dmx_inflate_parallel_plan_work(1, 0)
    if work_bytes is None:
        work_bytes = L.dmx_zindex_device_work(out_cap, max_points)
    return L.dmx_zindex_from_parallel_async(vp(plan), plan_bytes, vp(dec), vp(out), out_cap, max_live, span, vp(points), vp(adlers),
                                            vp(windows), max_points, vp(work), work_bytes, vp(status), vp(0))


def test_argument_errors():
    L = D.lib()
    for name in ("plan", "dec", "out", "points", "adlers", "windows", "work", "status"):
        assert _call(**{name: 0}) == INVAL, name                # a NULL pointer
    assert _call(plan=0x10080) == INVAL                        # 256-byte alignment of the plan
    assert _call(work=0x20080) == INVAL                        # ... of the work buffer
    assert _call(points=0x2004) == INVAL                       # 8-byte alignment of the points
    assert _call(status=0x7004) == INVAL                       # ... of the record
    assert _call(dec=0x5004) == INVAL                          # ... of the decode's record
    assert _call(adlers=0x6002) == INVAL                       # 4-byte alignment of the Adler-32s
    assert _call(plan_bytes=L.dmx_inflate_parallel_plan_work(1, 0) - 1) == INVAL
    assert _call(plan_bytes=0) == INVAL
    assert _call(work_bytes=L.dmx_zindex_device_work(0, 1) - 1) == INVAL
    assert _call(work_bytes=0) == INVAL
    assert _call(span=(1 << 30) + 1) == RANGE
    assert _call(span=(1 << 30) + 1, points=0) == INVAL        # what is refused first is the pointer
    # the host twin
    z, data = I.window_edge_stream()
    chunks, info = D.inflate_parallel_plan_host(z, chunk_bytes=1024)
    assert info["status"] == 0 and len(chunks) > 10
    assert G.twin(chunks, data, (1 << 30) + 1)[0] == RANGE
    assert G.twin(chunks[:0], data, 0)[0] == INVAL             # no chunk
    assert G.twin(chunks[:-1], data, 0)[0] == INVAL            # the chunks do not reach the end of the bytes
    assert G.twin(chunks, data[:-1], 0)[0] == INVAL            # ... or pass it
    assert G.twin(chunks[1:], data, 0)[0] == INVAL             # ... or do not begin at 0
    twin = D.lib().dmx_zindex_from_chunks_host
    p, a, w, n = vp(0), vp(0), vp(0), ctypes.c_uint32(0)
    ch = np.ascontiguousarray(chunks)
    args = (vp(ch.ctypes.data), len(ch), data, len(data), 0)
    assert twin(None, len(ch), data, len(data), 0, ctypes.byref(p), ctypes.byref(a), ctypes.byref(w), ctypes.byref(n)) == INVAL
    assert twin(args[0], len(ch), None, len(data), 0, ctypes.byref(p), ctypes.byref(a), ctypes.byref(w), ctypes.byref(n)) == INVAL
    assert twin(*args, None, ctypes.byref(a), ctypes.byref(w), ctypes.byref(n)) == INVAL
    assert twin(*args, ctypes.byref(p), None, ctypes.byref(w), ctypes.byref(n)) == INVAL
    assert twin(*args, ctypes.byref(p), ctypes.byref(a), None, ctypes.byref(n)) == INVAL
    assert twin(*args, ctypes.byref(p), ctypes.byref(a), ctypes.byref(w), None) == INVAL
    with pytest.raises(ValueError):
        D.inflate_parallel_indexed(z, fmt="bzip2")
    with pytest.raises(ValueError):
        D.inflate_parallel_indexed(z, span=(1 << 30) + 1)


def test_bound_and_work():
    L = D.lib()
    bound, work = L.dmx_zindex_points_bound, L.dmx_zindex_device_work
    # min(out_cap / span + 1, max_live), at least 1; span 0 is the default
    assert bound(0, 0, 0) == 1 and bound(0, 100, 1) == 1 and bound(1 << 30, 0, 1) == 1 and bound(1 << 30, 1, 1) == 1
    assert bound(100, 1000, 1) == 101 and bound(100, 50, 1) == 50 and bound(99, 1000, 100) == 1 and bound(100, 1000, 100) == 2
    assert bound(1 << 20, 1000, 0) == bound(1 << 20, 1000, D.DMX_ZINDEX_DEF_SPAN) == 5
    assert bound(0xFFFFFFF0, 0xFFFFFFFF, 1) == 0xFFFFFFF1 and bound(0xFFFFFFF0, 0xFFFFFFFF, 1 << 30) == 4
    caps = [0, 1, 65535, 65536, 65537, 1 << 20, (1 << 20) + 1, 100_000_000, 0xFFFFFFF0]
    lives = [0, 1, 2, 63, 64, 65, 1000, 1 << 20]
    for span in (1, 1000, 65536, 0, 1 << 30):
        for i, c in enumerate(caps):
            for j, n in enumerate(lives):
                b = bound(c, n, span)
                assert 1 <= b <= max(n, 1) and b <= c // (span or D.DMX_ZINDEX_DEF_SPAN) + 1
                assert i == 0 or b >= bound(caps[i - 1], n, span)
                assert j == 0 or b >= bound(c, lives[j - 1], span)
    # a multiple of 256, monotone in both, with room for the bases and 8 bytes a piece
    for i, c in enumerate(caps):
        for j, n in enumerate(lives):
            wb = work(c, n)
            assert wb % 256 == 0 and wb >= 256 + 4 * (n + 1) + 8 * (c // 65536 + n)
            assert i == 0 or wb >= work(caps[i - 1], n)
            assert j == 0 or wb >= work(c, lives[j - 1])
    assert work(0, 0) == 512 and work(0, 1) == 768


# ---- the host twin, pinned to zlib --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan(k, cut):
    name, z, fmt, data = I.round_trip_inputs()[k]
    chunks, info = D.inflate_parallel_plan_host(z, fmt="raw" if fmt == "raw" else "auto", chunk_bytes=cut)
    assert info["status"] == 0 and info["out_len"] == len(data) and info["nlive"] == len(chunks)
    return chunks, info


def index_of(chunks, info, data, span):
    """the host twin's index of a plan as a ZIndex"""
    r, points, adlers, windows = G.twin(chunks, data, span)
    assert r == 0
    return D.ZIndex(points, adlers, windows, info["format"], info["out_len"], info["in_used"], info["check"],
                    span or D.DMX_ZINDEX_DEF_SPAN)


@pytest.mark.parametrize("span", (1, 65536, 10 ** 9))
@pytest.mark.parametrize("cut", (1024, None))
@pytest.mark.parametrize("k", range(10))
def test_host_twin_is_true(k, cut, span):
    name, z, fmt, data = I.round_trip_inputs()[k]
    chunks, info = _plan(k, cut)
    ix = index_of(chunks, info, data, span)
    ZA.check_index(ix, z, data, fmt, shiftable="sync" not in name)
    nlive = len(chunks)
    assert ix.npoints <= D.lib().dmx_zindex_points_bound(len(data), nlive, span) == min(len(data) // span + 1, nlive)
    # every point is a run of whole chunks
    starts = {int(b): c for c, b in enumerate(chunks["bit"])}
    first = [starts[int(b)] for b in ix.points["bit"]]
    assert first[0] == 0 and first == sorted(set(first))
    for j, c in enumerate(first):
        stop = first[j + 1] if j + 1 < len(first) else nlive
        assert int(ix.points["out_off"][j]) == int(chunks["out_off"][c])
        assert int(ix.points["out_len"][j]) == int(chunks["out_len"][c:stop].sum())
        assert int(ix.points["end_bit"][j]) == int(chunks["end_bit"][stop - 1])
    if span == 10 ** 9:
        assert ix.npoints == 1
    if span == 1:   # every live chunk that follows output is a point: these chunks all produce some
        assert (chunks["out_len"][:-1] > 0).all() and ix.npoints == nlive
    if span == 65536:
        assert ix.npoints >= 10


def test_new_inputs():
    """what the GPU tests rely on in the two new streams, from the host plan"""
    z, data = G.sync3001_stream()
    chunks, info = D.inflate_parallel_plan_host(z, chunk_bytes=1024)
    assert info["status"] == 0 and info["nlive"] >= 50
    ix = index_of(chunks, info, data, 1)
    ZA.check_index(ix, z, data, "zlib", shiftable=False)
    off = ix.points["out_off"].astype(np.int64)
    assert set(int(o) & 15 for o in off) == set(range(16))          # the windows' sources at every residue mod 16
    assert int(((off > 0) & (off < W)).sum()) >= 5                   # windows with a zero prefix
    z, data = G.high16_stream()
    assert min(data) >= 0xF0 and len(data) == 1 << 20
    for cut in (1024, 4096, None):
        chunks, info = D.inflate_parallel_plan_host(z, chunk_bytes=cut)
        assert info["status"] == 0 and info["nlive"] >= 8
    ix = index_of(chunks, info, data, 262144)
    ZA.check_index(ix, z, data, "zlib")
    assert 3 <= ix.npoints <= 4 and int(ix.points["out_len"].max()) > 4 * 65536 - 65536   # points of several pieces
    # the sums a 64 KiB piece reaches: b before its reduction is within a factor 1.07 of its bound
    piece = np.frombuffer(data[:65536], dtype=np.uint8).astype(np.uint64)
    assert int((piece * np.arange(65536, 0, -1, dtype=np.uint64)).sum()) > 0.93 * 255 * 65536 * 65537 // 2


def test_selection_rule_asan_ubsan():
    """tests/c/zsel_model.cpp ends with `0 failed checks`: over 4 000 random chunk tables (chunks of no
    output, one chunk, spans from 1 to above the total) dmx_zs_select gives the points of a plain
    restatement of the host builder's loop, they tile the chunks, hold span bytes each but the last,
    stay below the bound, and a capacity below npoints writes nothing beyond it."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.zsel"])
    exe = os.path.join(REPO, "build", "c", "zsel_model")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert " checks, 0 failed checks" in p.stdout
    m = re.search(r"(\d+) chunk tables", p.stdout)
    assert m and int(m.group(1)) >= 4000
