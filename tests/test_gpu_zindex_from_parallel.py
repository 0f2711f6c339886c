"""The seek-point index from the one-pass decode on the device (dmx_zindex_from_parallel_async,
zindex_from_parallel_async, inflate_parallel_indexed): the device's three arrays against the host
twin's byte for byte and against zlib (check_index of test_zindex_api.py), the decode through the
index, Adler-32 per point for every format, the bytes behind npoints entries, the two-call idiom,
a decode record with a status, range reads, plan + decode + index in one graph, the Python call."""
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
import inflate_parallel_dev_inputs as P
import inflate_parallel_inputs as I
import test_zindex_api as ZA
import zindex_gpu_inputs as G

pytestmark = pytest.mark.gpu

E = D.E
SZ, HUFDIS, ZADL32 = -E["E_SZ"], -E["E_HUFDIS"], -E["E_ZADL32"]
FMT = {"auto": 0, "zlib": 1, "gzip": 2, "raw": 3}
CANARY = 0xA5
GUARD = 2     # entries behind max_points in every array
W = 32768
NAMES = ["l1-zlib", "l1-gzip", "l1-raw", "l6-zlib", "l6-gzip", "l6-raw", "l9-zlib", "l9-gzip", "l9-raw", "l6-zlib-sync3000",
         "sync3001", "high16", "run", "edge"]
_streams = {}


def stream(name):
    """(name, stream, fmt, data, chunk_bytes) of G.streams()"""
    if not _streams:
        _streams.update({s[0]: s for s in G.streams()})
        assert list(_streams) == NAMES
    return _streams[name]


def on_device(z):
    buf = torch.zeros(len(z) + 8, dtype=torch.uint8, device="cuda")
    buf[:len(z)] = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    return buf[:len(z)]


def par_record(t):
    return D.ParStatus.from_buffer_copy(t.cpu().numpy().tobytes()[:56])


def decoded(z, fmt, chunk, verify=True, max_live=None):
    """plan and decode of z on the device: (zt, plan, the decode's record tensor, its record, out, the plan's chunks)"""
    L = D.lib()
    zt = on_device(z)
    plan = torch.full((L.dmx_inflate_parallel_plan_work(len(z), chunk),), 0x5A, dtype=torch.uint8, device="cuda")
    assert D.inflate_parallel_plan_async(zt, FMT["raw" if fmt == "raw" else "auto"], chunk, plan) == 0
    rec = par_record(plan[:56])
    chunks = plan[256:256 + 32 * rec.nlive].cpu().numpy().view(D.PCHUNK_DTYPE) if not rec.status else None
    cap = max(int(rec.out_len), 1)
    out = torch.full((cap,), 0x33, dtype=torch.uint8, device="cuda")
    work = torch.empty(max(int(rec.work_len), 256), dtype=torch.uint8, device="cuda")
    st = torch.full((7,), -1, dtype=torch.int64, device="cuda")
    assert D.inflate_parallel_decode_async(zt, plan, rec.nlive if max_live is None else max_live, out, rec.out_len, work, verify,
                                           st) == 0
    return zt, plan, st, par_record(st), out, chunks


class Arrays:
    """the three arrays and the record, every byte the canary, with GUARD entries behind max_points"""

    def __init__(self, max_points):
        n = max_points + GUARD
        self.max_points = max_points
        self.points = torch.full((n, 32), CANARY, dtype=torch.uint8, device="cuda")
        self.adlers = torch.full((n, 4), CANARY, dtype=torch.uint8, device="cuda")
        self.windows = torch.full((n, W), CANARY, dtype=torch.uint8, device="cuda")
        self.status = torch.full((5,), -1, dtype=torch.int64, device="cuda")

    def record(self):
        return D.ZIndexStatus.from_buffer_copy(self.status.cpu().numpy().tobytes())

    def host(self, n):
        return (self.points[:n].cpu().numpy().reshape(-1).view(D.PCHUNK_DTYPE), self.adlers[:n].cpu().numpy().reshape(-1).view(np.uint32),
                self.windows[:n].cpu().numpy())

    def untouched(self, n=0):
        """every byte from entry n on still holds the canary"""
        return all(bool((t[n:] == CANARY).all()) for t in (self.points, self.adlers, self.windows))


def index_dev(plan, st, out, out_cap, max_live, span, max_points, work_bytes=None):
    L = D.lib()
    arr = Arrays(max_points)
    wb = L.dmx_zindex_device_work(out_cap, max_points) if work_bytes is None else work_bytes
    work = torch.empty(max(wb, 256), dtype=torch.uint8, device="cuda")
    r = D.zindex_from_parallel_async(plan, st, out, out_cap, max_live, span, arr.points, arr.adlers, arr.windows, max_points,
                                     work[:wb], arr.status)
    assert r == 0
    return arr, arr.record()


def built(name, span):
    """the device index of a stream of G.streams() and everything around it"""
    _, z, fmt, data, chunk = stream(name)
    zt, plan, st, rec, out, chunks = decoded(z, fmt, chunk)
    assert rec.status == 0 and rec.out_len == len(data) and rec.nlive == len(chunks) > 1
    assert out.cpu().numpy().tobytes() == data
    cap = D.lib().dmx_zindex_points_bound(rec.out_len, rec.nlive, span)
    arr, zrec = index_dev(plan, st, out, rec.out_len, rec.nlive, span, cap)
    return z, fmt, data, zt, plan, st, rec, out, chunks, arr, zrec


def as_index(arr, zrec):
    return D.ZIndex(*arr.host(zrec.npoints), zrec.format, zrec.out_len, zrec.in_used, zrec.check, zrec.span)


# ---- the whole path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("span", (1, 65536, 0))
@pytest.mark.parametrize("name", NAMES)
def test_device_index_is_the_host_twins(name, span):
    z, fmt, data, zt, plan, st, rec, out, chunks, arr, zrec = built(name, span)
    assert (zrec.status, zrec.format, zrec.out_len, zrec.in_used, zrec.check, zrec.span, zrec.reserved) == \
        (0, rec.format, rec.out_len, rec.in_used, rec.check, span or D.DMX_ZINDEX_DEF_SPAN, 0)
    r, points, adlers, windows = G.twin(chunks, data, span)
    assert r == 0 and zrec.npoints == len(points)
    got = arr.host(zrec.npoints)
    assert got[0].tobytes() == points.tobytes()
    assert got[1].tobytes() == adlers.tobytes()
    assert np.array_equal(got[2], windows)
    assert arr.untouched(zrec.npoints)                       # no byte behind npoints entries
    assert out.cpu().numpy().tobytes() == data               # d_out is read, never written
    assert plan[256:256 + 32 * rec.nlive].cpu().numpy().tobytes() == chunks.tobytes()
    ix = as_index(arr, zrec)
    ZA.check_index(ix, z, data, fmt, shiftable="sync" not in name)
    assert D.inflate_indexed(zt, ix, verify=True).cpu().numpy().tobytes() == data
    if name == "sync3001" and span == 1:
        off = ix.points["out_off"].astype(np.int64)
        assert set(int(o) & 15 for o in off) == set(range(16)) and int(((off > 0) & (off < W)).sum()) >= 5
    if name == "high16" and span == 0:
        assert ix.npoints >= 3 and int(ix.points["out_len"].max()) > 3 * 65536


def test_every_format_carries_adler32_per_point():
    for name in ("l6-gzip", "l6-raw", "l6-zlib"):
        z, fmt, data, zt, plan, st, rec, out, chunks, arr, zrec = built(name, 100_000)
        assert zrec.status == 0 and zrec.npoints >= 5
        want = {"gzip": zlib.crc32(data), "raw": 0, "zlib": zlib.adler32(data)}[fmt]
        assert zrec.check == want and zrec.format == FMT[fmt]
        points, adlers, _ = arr.host(zrec.npoints)
        for k in range(zrec.npoints):
            o, n = int(points["out_off"][k]), int(points["out_len"][k])
            assert int(adlers[k]) == zlib.adler32(data[o:o + n]), (name, k)


# ---- the two-call idiom -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sync3001", "l6-zlib-sync3000"])
def test_capacities_too_small(name):
    span = 1
    z, fmt, data, zt, plan, st, rec, out, chunks, arr, zrec = built(name, span)
    n = zrec.npoints
    need = D.lib().dmx_zindex_device_work(rec.out_len, n)
    assert zrec.status == 0 and n >= 2 and need - 256 >= D.lib().dmx_zindex_device_work(0, 1)
    for what, (mp, wb) in (("max_points", (n - 1, D.lib().dmx_zindex_device_work(rec.out_len, n))),
                           ("work_bytes", (n, need - 256))):
        a2, r2 = index_dev(plan, st, out, rec.out_len, rec.nlive, span, mp, wb)
        assert (r2.status, r2.npoints, r2.format, r2.span) == (SZ, n, rec.format, span or D.DMX_ZINDEX_DEF_SPAN), what
        assert a2.untouched(), what
    a3, r3 = index_dev(plan, st, out, rec.out_len, rec.nlive, span, n, need)   # and the exact numbers pass
    assert r3.status == 0 and r3.npoints == n and a3.untouched(n)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a3.host(n), arr.host(n)))
    # larger capacities than the decode's numbers change nothing
    a4, r4 = index_dev(plan, st, out, rec.out_len, rec.nlive + 7, span, n + 5)
    assert r4.status == 0 and r4.npoints == n and a4.untouched(n)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a4.host(n), arr.host(n)))


# ---- a decode record with a status ------------------------------------------------------------------
def _propagated(z, fmt, chunk, want, max_live=None, span=4096):
    zt, plan, st, rec, out, chunks = decoded(z, fmt, chunk, max_live=max_live)
    assert rec.status == want, (rec.status, want)
    arr, zrec = index_dev(plan, st, out, out.numel(), 1000, span, 50)
    assert (zrec.status, zrec.format, zrec.span) == (want, rec.format, span)
    assert (zrec.out_len, zrec.in_used, zrec.check, zrec.npoints, zrec.reserved) == (0, 0, 0, 0, 0)
    assert arr.untouched()


def test_a_decode_status_is_copied():
    for name, z, _ in P.too_far_streams():
        _propagated(z, "zlib", 1024, HUFDIS)
    z = bytearray(stream("l6-zlib")[1])
    z[-1] ^= 1
    _propagated(bytes(z), "zlib", 4096, ZADL32)
    _, z, fmt, data, chunk = stream("l6-gzip")
    nlive = D.inflate_parallel_plan_host(z, chunk_bytes=chunk)[1]["nlive"]
    _propagated(z, fmt, chunk, SZ, max_live=nlive - 1)


# ---- range reads ------------------------------------------------------------------------------------
def test_range_reads_with_the_device_index():
    z, fmt, data, zt, plan, st, rec, out, chunks, arr, zrec = built("l6-zlib-sync3000", 65536)
    ix = as_index(arr, zrec)
    rng = np.random.default_rng(77)
    off = rng.integers(0, len(data), size=64)
    ln = np.minimum(rng.integers(0, 200_000, size=64), len(data) - off)
    got, offsets = D.zindex_read_ranges(zt, ix, np.stack([off, ln], axis=1))
    h, o = got.cpu().numpy().tobytes(), offsets.cpu().numpy()
    for q in range(64):
        assert h[o[q]:o[q + 1]] == data[off[q]:off[q] + ln[q]], q
    assert D.zindex_pread(zt, ix, len(data) - 5000, 5000).cpu().numpy().tobytes() == data[-5000:]


# ---- in a graph -------------------------------------------------------------------------------------
def test_plan_decode_and_index_in_a_graph():
    """plan + decode + index captured once with capacities, replayed on two different streams of one
    length copied into the same tensor, and on the first again"""
    t = I.text()
    a, b = t[:300_000], t[310_000:590_000]
    za, zb = I.deflate(a, 6, 15, flush_every=5000), I.deflate(b, 9, 15, flush_every=5000)   # 60 and 56 live chunks, 10 points each
    n = max(len(za), len(zb)) + 16
    za, zb = za + bytes(n - len(za)), zb + bytes(n - len(zb))   # bytes behind the trailer are ignored
    chunk, cap, span = 1024, 300_000 + 100, 30_000
    L = D.lib()
    nc = -(-n // chunk)
    mp = L.dmx_zindex_points_bound(cap, nc, span)
    zt = torch.zeros(n, dtype=torch.uint8, device="cuda")
    plan = torch.zeros(L.dmx_inflate_parallel_plan_work(n, chunk), dtype=torch.uint8, device="cuda")
    work = torch.zeros(L.dmx_inflate_parallel_work(cap, nc), dtype=torch.uint8, device="cuda")
    zwork = torch.zeros(L.dmx_zindex_device_work(cap, mp), dtype=torch.uint8, device="cuda")
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    st = torch.zeros(7, dtype=torch.int64, device="cuda")
    arr = Arrays(mp)

    def enqueue():
        r = D.inflate_parallel_plan_async(zt, 0, chunk, plan)
        r = r or D.inflate_parallel_decode_async(zt, plan, nc, out, cap, work, True, st)
        return r or D.zindex_from_parallel_async(plan, st, out, cap, nc, span, arr.points, arr.adlers, arr.windows, mp, zwork,
                                                 arr.status)

    zt.copy_(torch.frombuffer(bytearray(za), dtype=torch.uint8))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the kernels are loaded before the capture
        assert enqueue() == 0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r = enqueue()
    assert r == 0
    for z, data in ((zb, b), (za, a), (zb, b)):
        zt.copy_(torch.frombuffer(bytearray(z), dtype=torch.uint8))
        for x in (arr.points, arr.adlers, arr.windows):
            x.fill_(CANARY)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        rec, zrec = par_record(st), arr.record()
        assert (rec.status, zrec.status) == (0, 0) and zrec.out_len == len(data) and zrec.npoints >= 5
        chunks = plan[256:256 + 32 * rec.nlive].cpu().numpy().view(D.PCHUNK_DTYPE)
        r, points, adlers, windows = G.twin(chunks, data, span)
        got = arr.host(zrec.npoints)
        assert r == 0 and got[0].tobytes() == points.tobytes() and got[1].tobytes() == adlers.tobytes()
        assert np.array_equal(got[2], windows) and arr.untouched(zrec.npoints)
        ZA.check_index(as_index(arr, zrec), z, data, "zlib", shiftable=False)   # (sync flushes)


# ---- the Python call --------------------------------------------------------------------------------
def test_inflate_parallel_indexed(monkeypatch):
    _, z, fmt, data, chunk = stream("l6-zlib")
    zt = on_device(z)
    info = {}
    out, ix = D.inflate_parallel_indexed(zt, chunk_bytes=chunk, span=100_000, info=info)
    assert (info["route"], info["index_route"], info["status"]) == ("parallel", "device", 0) and info["npoints"] == ix.npoints >= 5
    assert out.cpu().numpy().tobytes() == data
    ZA.check_index(ix, z, data, fmt)
    assert (ix.span, ix.in_used) == (100_000, len(z))
    # the cache is seeded: nothing of the index is uploaded again
    dev = torch.device("cuda", torch.cuda.current_device())
    assert dev in ix._dev and ix.cuda() is ix._dev[dev]
    pt, at, wt = ix.cuda()
    assert (tuple(pt.shape), pt.dtype, tuple(at.shape), at.dtype, tuple(wt.shape), wt.dtype) == \
        ((ix.npoints, 4), torch.int64, (ix.npoints,), torch.int32, (ix.npoints, W), torch.uint8)
    uploads = []
    real = torch.from_numpy
    monkeypatch.setattr(torch, "from_numpy", lambda a: (uploads.append(a.nbytes), real(a))[1])
    assert D.inflate_indexed(zt, ix).cpu().numpy().tobytes() == data
    assert D.zindex_pread(zt, ix, 700_000, 9000).cpu().numpy().tobytes() == data[700_000:709_000]
    assert max(uploads, default=0) < 1024   # (the offsets and selections of a read, never the 32 KiB windows)
    monkeypatch.undo()
    # bytes, the default cut and span
    out, jx = D.inflate_parallel_indexed(z)
    assert out.cpu().numpy().tobytes() == data and jx.span == D.DMX_ZINDEX_DEF_SPAN and jx.npoints >= 3
    ZA.check_index(jx, z, data, fmt)
    # the serial route: the index comes from the host
    z, data = I.stored_only_stream()
    info = {}
    out, ix = D.inflate_parallel_indexed(on_device(z), chunk_bytes=1024, span=12000, info=info)
    assert (info["route"], info["index_route"]) == ("serial", "host") and ix.npoints == info["npoints"] == 4
    assert out.cpu().numpy().tobytes() == data
    ZA.check_index(ix, z, data, "zlib")
    assert D.inflate_indexed(on_device(z), ix).cpu().numpy().tobytes() == data
    # a stream with a status raises it
    bad = bytearray(stream("l6-zlib")[1])
    bad[-1] ^= 1
    with pytest.raises(D.DeflateError) as e:
        D.inflate_parallel_indexed(bytes(bad), chunk_bytes=4096)
    assert e.value.code == ZADL32
