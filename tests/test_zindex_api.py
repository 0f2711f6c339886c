"""The seek-point index of one foreign stream, on the host (dmx_zindex_build_host, ZIndex): the
exports and their declarations, the struct, the argument errors, the index pinned to zlib's own
verdict on every point (check_points here, and inflate_parallel_inputs.check_chunks wherever no
stored block lies behind an odd bit), its Adler-32s and windows, the
statuses pinned to deflate_decompress, save / load, and the builder under the sanitizers
(tests/c/zindex_model.cpp: ASan + UBSan, a stand-alone program)."""
import ctypes
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import deflate_compression_amd as D
import deflate_craft as C
import inflate_parallel_inputs as I

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE = -E["E_INVAL"], -E["E_RANGE"]
vp = ctypes.c_void_p
CALLS = ("dmx_zindex_build_host", "dmx_inflate_points_work", "dmx_inflate_points_async")
W = 32768


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in CALLS:
        f = getattr(L, name)
        assert f.argtypes is not None, name
        assert name + "(" in hdr, name
    for name in ("dmx_zpoint", "dmx_zindex_status", "seek points", "DMX_ZINDEX_DEF_SPAN"):
        assert name in hdr, name
    for name in ("ZIndex", "ZIndexStatus", "zindex_build", "inflate_points_async", "inflate_indexed", "zindex_read_ranges",
                 "zindex_pread", "DMX_ZINDEX_WINDOW", "DMX_ZINDEX_DEF_SPAN", "DMX_ZINDEX_MAX_SPAN"):
        assert name in D.__all__ and hasattr(D, name), name
    # the ctypes signatures have the header's argument counts
    for name in CALLS:
        decl = re.search(r"^\w+\s+" + name + r"\(([^;]*?)\);", hdr, re.S | re.M).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(getattr(L, name).argtypes) == len([a for a in decl.split(",") if a.strip() not in ("", "void")]), name


def test_struct_sizes_and_constants():
    assert ctypes.sizeof(D.ZIndexStatus) == 40
    assert [getattr(D.ZIndexStatus, f).offset for f, _ in D.ZIndexStatus._fields_] == [0, 4, 8, 16, 24, 28, 32, 36]
    assert "/* 40 bytes */" in open(os.path.join(REPO, "include", "dmx.h")).read()
    assert (D.DMX_ZINDEX_WINDOW, D.DMX_ZINDEX_DEF_SPAN, D.DMX_ZINDEX_MAX_SPAN) == (32768, 262144, 1 << 30)
    assert D.lib().dmx_inflate_points_work(7) == D.lib().dmx_inflate_batch_work(7)


def test_argument_errors():
    host = D.lib().dmx_zindex_build_host
    rec = D.ZIndexStatus()
    p, a, w = vp(0), vp(0), vp(0)
    args = (ctypes.byref(p), ctypes.byref(a), ctypes.byref(w))
    z = zlib.compress(b"abc")
    assert host(None, 10, 0, 0, *args, ctypes.byref(rec)) == INVAL
    assert host(z, len(z), 0, 0, *args, None) == INVAL
    assert host(z, len(z), 0, 0, None, args[1], args[2], ctypes.byref(rec)) == INVAL
    assert host(z, len(z), 0, 0, args[0], None, args[2], ctypes.byref(rec)) == INVAL
    assert host(z, len(z), 0, 0, args[0], args[1], None, ctypes.byref(rec)) == INVAL
    assert host(z, len(z), 4, 0, *args, ctypes.byref(rec)) == INVAL
    assert host(z, len(z), 0, (1 << 30) + 1, *args, ctypes.byref(rec)) == RANGE
    assert (p.value, a.value, w.value) == (None, None, None)
    with pytest.raises(ValueError):
        D.zindex_build(z, fmt="bzip2")
    with pytest.raises(ValueError):
        D.zindex_build(z, span=(1 << 30) + 1)
    ix = D.zindex_build(z, span=1 << 30)
    assert ix.span == 1 << 30 and ix.npoints == 1
    assert D.zindex_build(z).span == D.DMX_ZINDEX_DEF_SPAN


def _points_call(z=0x1000, zbytes=64, points=0x2000, adler=0x6000, windows=0x8000, npoints=3, sel=0x7000, dst=0x9000, n=3,
                 out=0x3000, out_bytes=64, results=0x4000, work=0x10000, work_bytes=None, status=0x5000):
    """dmx_inflate_points_async on made-up addresses: an argument error returns before they are used"""
    L = D.lib()
    if work_bytes is None:
        work_bytes = L.dmx_inflate_points_work(n)
    return L.dmx_inflate_points_async(vp(z), zbytes, vp(points), vp(adler), vp(windows), npoints, vp(sel), vp(dst), n, vp(out),
                                      out_bytes, vp(results), vp(work), work_bytes, vp(status), vp(0))


def test_points_argument_errors():
    """the checks before any device call, as dmx_inflate_batch_async's table (test_inflate_batch_api.py)"""
    need = D.lib().dmx_inflate_points_work(3)
    assert _points_call(results=0) == INVAL
    assert _points_call(status=0) == INVAL
    assert _points_call(work=0) == INVAL
    assert _points_call(points=0) == INVAL                 # NULL with nsel > 0
    assert _points_call(windows=0) == INVAL
    assert _points_call(out=0) == INVAL
    assert _points_call(z=0) == INVAL                      # NULL with zbytes > 0
    assert _points_call(points=0x2004) == INVAL            # 8-byte alignment of the points
    assert _points_call(dst=0x9004) == INVAL               # ... of the destinations
    assert _points_call(results=0x4004) == INVAL           # ... of the results
    assert _points_call(status=0x5004) == INVAL            # ... of the record
    assert _points_call(adler=0x6002) == INVAL             # 4-byte alignment of the Adler-32s
    assert _points_call(sel=0x7002) == INVAL               # ... of the selection
    assert _points_call(work=0x10080) == INVAL             # 256-byte alignment of the work buffer
    assert _points_call(work_bytes=need - 1) == INVAL
    assert _points_call(work_bytes=0) == INVAL
    # the optional arrays may be NULL: what is refused then is the next thing wrong, not they
    assert _points_call(adler=0, sel=0, dst=0, status=0) == INVAL
    assert _points_call(n=0, points=0, windows=0, out=0, work_bytes=need, work=0x10080) == INVAL


# ---- the index, pinned to zlib -------------------------------------------------------------------

def _body_bit(z, fmt):
    if fmt == "raw":
        return 0
    if fmt == "zlib":
        return 16
    assert z[3] == 0   # (a plain gzip header, as Python's zlib writes it)
    return 80


def check_points(z, data, points, body_bit):
    """I.check_chunks for points that begin at any bit: the same verdict of zlib on every point --
    the points tile the output and follow one another in the stream, and bits [bit, end_bit) of each,
    behind the 32 KiB of output in front of it and in front of an empty final block, are whole blocks
    that inflate to exactly that point's bytes -- with the bits kept at their own residue in the byte.
    check_chunks shifts a chunk to bit 0, which moves the padding of every stored block in it unless
    bit & 7 == 0; a point behind a sync flush begins with a stored block at any residue.  Here empty
    blocks in front (one dynamic block of 111 bits for an odd residue, fixed blocks of 10 bits) bring
    zlib to bit & 7 first, and the point's bytes follow as they lie in the stream."""
    assert len(points) >= 1 and int(points["bit"][0]) == body_bit and int(points["out_off"][0]) == 0
    off = 0
    for k in range(len(points)):
        bit, end, o, n = (int(points[f][k]) for f in ("bit", "end_bit", "out_off", "out_len"))
        assert o == off and end > bit, (k, o, off)
        if k + 1 < len(points):
            assert int(points["bit"][k + 1]) == end, k
        d, r = C.Deflate(), bit & 7
        if r & 1:
            I._block(d, [])
        while d.bitpos & 7 != r:
            d.fixed_block([("L", 256)], False)
        lo, hi = bit >> 3, end >> 3
        if lo == hi:
            d.bits((z[lo] >> r) & ((1 << (end - bit)) - 1), end - bit)
        else:
            d.bits(z[lo] >> r, 8 - r)
            assert d.n == 0
            d.buf += z[lo + 1:hi]
            if end & 7:
                d.bits(z[hi] & ((1 << (end & 7)) - 1), end & 7)
        d.bits(0b0000000_01_1, 10)   # BFINAL = 1, BTYPE = 01, the 7-bit end-of-block code
        dec = zlib.decompressobj(-15, zdict=data[max(0, o - 32768):o]) if o else zlib.decompressobj(-15)
        got = dec.decompress(d.getvalue())
        assert dec.eof and got == data[o:o + n], (k, bit, end, len(got), n)
        off += n
    assert off == len(data)


def check_index(ix, z, data, fmt, shiftable=True):
    """everything an index promises, against zlib and the data.  shiftable: no point of it holds a
    stored block behind a bit that is not a multiple of 8, so I.check_chunks can judge it too."""
    assert ix.format == {"zlib": 1, "gzip": 2, "raw": 3}[fmt]
    assert ix.out_len == len(data) and ix.npoints == len(ix.points) == len(ix.adlers) == len(ix.windows)
    want = {"zlib": lambda: int.from_bytes(z[ix.in_used - 4:ix.in_used], "big"),
            "gzip": lambda: int.from_bytes(z[ix.in_used - 8:ix.in_used - 4], "little"), "raw": lambda: 0}[fmt]()
    assert ix.check == want
    check_points(z, data, ix.points, _body_bit(z, fmt))
    if shiftable:
        I.check_chunks(z, data, ix.points, _body_bit(z, fmt))
    assert ix.windows.shape == (ix.npoints, W) and ix.windows.dtype == np.uint8 and ix.adlers.dtype == np.uint32
    for k in range(ix.npoints):
        o, n = int(ix.points["out_off"][k]), int(ix.points["out_len"][k])
        assert int(ix.adlers[k]) == zlib.adler32(data[o:o + n]), k
        wlen = min(o, W)
        assert ix.windows[k, W - wlen:].tobytes() == data[o - wlen:o], k
        assert not ix.windows[k, :W - wlen].any(), k
    # a point ends at the first boundary at which it holds span bytes: all but the last are that long
    assert (ix.points["out_len"][:-1] >= min(ix.span, max(len(data), 1))).all()


@pytest.mark.parametrize("span", (1, 65536, 10 ** 9))
@pytest.mark.parametrize("k", range(10))
def test_index_is_true(k, span):
    name, z, fmt, data = I.round_trip_inputs()[k]
    ix = D.zindex_build(z, fmt="raw" if fmt == "raw" else "auto", span=span)
    assert ix.in_used == len(z) and ix.span == span
    # (the sync-flush stream's points hold stored blocks behind any bit: check_points alone judges them)
    check_index(ix, z, data, fmt, shiftable="sync" not in name)
    if span == 10 ** 9:
        assert ix.npoints == 1
    if span == 65536:
        assert ix.npoints >= 10 and int(ix.points["out_len"].max()) < 65536 + 200_000
    if span == 1 and "sync" in name:
        assert ix.npoints >= 400
        # a property of the input alone: the points of this stream start at every bit of a byte
        assert set(int(b) & 7 for b in ix.points["bit"]) == set(range(8))


def test_crafted_streams():
    z, data = I.window_edge_stream()
    ix = D.zindex_build(z, span=1)
    assert ix.npoints == 20 + 30
    check_index(ix, z, data, "zlib")
    z, data = I.stored_only_stream()
    for span in (1, 12000):
        ix = D.zindex_build(z, span=span)
        assert ix.npoints == (10 if span == 1 else 4)
        check_index(ix, z, data, "zlib")
    z, data = I.fixed_only_stream()
    ix = D.zindex_build(z, span=1)
    assert ix.npoints == 1   # one block: one point, whatever the span
    check_index(ix, z, data, "zlib")
    for payload in (3000, 30000):   # the exact builder indexes what the speculative plan gives up on
        z, data = I.false_candidate_stream(payload)
        ix = D.zindex_build(z, span=1)
        assert ix.npoints >= 20 and int(ix.points["out_len"][0]) == len(data) - 60_000   # the stored block, payload and all
        check_index(ix, z, data, "zlib", shiftable=False)   # (sync flushes behind the payload)


def test_zeros_and_empty():
    data = bytes(16 << 20)
    z = zlib.compress(data, 6)   # blocks of about 4.2 MB: the host plan refuses this stream
    _, info = D.inflate_parallel_plan_host(z)
    assert info["gave_up"] == 1
    ix = D.zindex_build(z, span=1 << 20)
    assert ix.npoints >= 3 and 4_000_000 < int(ix.points["out_len"][:-1].min()) and int(ix.points["out_len"].max()) < 4_400_000
    assert ix.in_used == len(z)
    check_index(ix, z, data, "zlib")
    for fmt, wbits in (("zlib", 15), ("gzip", 31), ("raw", -15)):
        z = I.deflate(b"", 6, wbits)
        ix = D.zindex_build(z, fmt="raw" if fmt == "raw" else "auto", span=1)
        assert (ix.npoints, ix.out_len, ix.in_used, int(ix.points["out_len"][0])) == (1, 0, len(z), 0)
        check_index(ix, z, b"", fmt)


def test_statuses_are_deflate_decompress():
    z = I.round_trip_inputs()[3][1]
    for bad, want in ((b"", "E_ZHEAD"), (b"\x78", "E_ZHEAD"), (b"\x77\x9c" + z[2:], "E_ZCMPMT"), (z[:1000], "E_LEN"),
                      (z[:-2], "E_ZADL32"), (z[:-1] + bytes([z[-1] ^ 1]), "E_ZADL32"), (b"\x78\xbb" + z[2:], "E_ZPDICT")):
        with pytest.raises(D.DeflateError) as e:
            D.deflate_decompress(bad)
        assert e.value.code == -E[want]
        with pytest.raises(D.DeflateError) as e2:
            D.zindex_build(bad, span=4096)
        assert e2.value.code == e.value.code, want
    g = I.round_trip_inputs()[4][1]
    assert g[:2] == b"\x1f\x8b"
    for bad in (g[:-3], g[:-8] + bytes([g[-8] ^ 1]) + g[-7:], g[:-4] + bytes([g[-4] ^ 1]) + g[-3:], g[:2] + b"\x07" + g[3:],
                g[:3] + b"\x80" + g[4:], g[:5000]):
        with pytest.raises(D.DeflateError) as e:
            D.deflate_decompress(bad)
        with pytest.raises(D.DeflateError) as e2:
            D.zindex_build(bad)
        assert e2.value.code == e.value.code, len(bad)
    with pytest.raises(D.DeflateError) as e:
        D.zindex_build(z, fmt="gzip")
    assert e.value.code == -E["E_ZHEAD"]
    # the record of a refused stream: a status and no index
    rec = D.ZIndexStatus()
    p, a, w = vp(1), vp(1), vp(1)
    assert D.lib().dmx_zindex_build_host(z, 1000, 0, 0, ctypes.byref(p), ctypes.byref(a), ctypes.byref(w), ctypes.byref(rec)) == 0
    assert (rec.status, rec.out_len, rec.in_used, rec.check, rec.npoints) == (-E["E_LEN"], 0, 0, 0, 0)
    assert (p.value, a.value, w.value) == (None, None, None)
    # trailing junk is ignored, and in_used says where it starts
    for k in (3, 4, 5):
        name, s, fmt, data = I.round_trip_inputs()[k]
        ix = D.zindex_build(s + b"junk" * 5, fmt="raw" if fmt == "raw" else "auto", span=100_000)
        assert ix.in_used == len(s) and ix.out_len == len(data), name
        check_index(ix, s + b"junk" * 5, data, fmt)


def test_save_and_load(tmp_path):
    name, z, fmt, data = I.round_trip_inputs()[4]
    ix = D.zindex_build(z, span=200_000)
    path = tmp_path / "index.npz"
    ix.save(path)
    jx = D.ZIndex.load(path)
    assert np.array_equal(ix.points, jx.points) and jx.points.dtype == np.dtype(D.PCHUNK_DTYPE)
    assert np.array_equal(ix.adlers, jx.adlers) and np.array_equal(ix.windows, jx.windows)
    assert (ix.format, ix.out_len, ix.in_used, ix.check, ix.span) == (jx.format, jx.out_len, jx.in_used, jx.check, jx.span)
    assert jx.npoints == ix.npoints >= 7 and jx.nbytes == ix.npoints * (32 + 4 + W)
    check_index(jx, z, data, fmt)


def test_host_twin_asan_ubsan(tmp_path):
    """tests/c/zindex_model.cpp ends with `0 failed checks`: over the round-trip streams, every cut
    point of two small ones and 10 000 mutations, the builder has deflate_decompress's status, its
    points tile the stream and the output, and every point, decoded again from its window alone by a
    plain restatement of RFC 1951, gives the bytes and the Adler-32 the index names -- with nothing
    read or written outside a buffer."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.zindex"])
    exe = os.path.join(REPO, "build", "c", "zindex_model")
    t = I.text()
    files = [("a-small-zlib", I.deflate(t[:1500], 6, 15, flush_every=400)),
             ("b-small-raw", I.deflate(t[5000:6200], 9, -15, flush_every=500))]
    files += [(name, z) for name, z, _, _ in I.round_trip_inputs()]
    files += [("edge-zlib", I.window_edge_stream()[0]), ("stored-zlib", I.stored_only_stream()[0])]
    paths = []
    for name, z in files:
        p = tmp_path / (name + ".bin")
        p.write_bytes(z)
        paths.append(str(p))
    p = subprocess.run([exe] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert " checks, 0 failed checks" in p.stdout
    m = re.search(r"(\d+) indexes, (\d+) points decoded again", p.stdout)
    assert m and int(m.group(1)) > 40 and int(m.group(2)) > 3000
    print(p.stdout.splitlines()[-2])
