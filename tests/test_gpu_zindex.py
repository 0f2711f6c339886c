"""Seek points on the GPU (dmx_inflate_points_async, csrc/dmx_inflate_dev.hip; inflate_indexed,
zindex_read_ranges, zindex_pread): one foreign stream, indexed once on the host (zindex_build), decoded
a wave per point.  Python's zlib gives the data; the index under test is the host builder's, which
tests/test_zindex_api.py pins to zlib.  Every input is at most 1.5 MB decoded, every output buffer
lies between canaries.  Streams of long zero runs are in tests/test_gpu_refill.py."""
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
import deflate_craft as C
import inflate_parallel_inputs as I

pytestmark = pytest.mark.gpu

E = {k: -v for k, v in D.E.items()}
CANARY = 0xA5
GUARD = 64
W = 32768
_cache = {}


def index_of(key, z, **kw):
    if key not in _cache:
        _cache[key] = D.zindex_build(z, **kw)
    return _cache[key]


def launch(z, points, adlers, windows, sel=None, dst=None, out_bytes=None, zbytes=None):
    """One call on fresh buffers, the output between GUARD canaries: (results, the output with its
    guards as numpy, BatchStatus).  adlers None: no verification.  The records start poisoned."""
    L = D.lib()
    npoints = len(points)
    n = npoints if sel is None else len(sel)
    if out_bytes is None:
        out_bytes = int(points["out_len"].sum())
    zt = torch.frombuffer(bytearray(z or b"\0"), dtype=torch.uint8).cuda()
    pt = torch.from_numpy(np.ascontiguousarray(points).view("<i8").reshape(-1, 4).copy()).cuda()
    at = None if adlers is None else torch.from_numpy(np.ascontiguousarray(adlers, dtype=np.uint32).view(np.int32).copy()).cuda()
    wt = torch.from_numpy(np.ascontiguousarray(windows)).cuda()
    st_ = None if sel is None else torch.from_numpy(np.asarray(sel, dtype=np.uint32).view(np.int32).copy()).cuda()
    dt = None if dst is None else torch.from_numpy(np.asarray(dst, dtype=np.uint64).view(np.int64).copy()).cuda()
    res = torch.full((max(n, 1) * 4,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(int(L.dmx_inflate_points_work(n)), dtype=torch.uint8, device="cuda")
    big = torch.full((GUARD + max(out_bytes, 1) + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    r = D.inflate_points_async(zt[:len(z) if zbytes is None else zbytes], pt, at, wt, npoints, st_, dt, n,
                               big[GUARD:GUARD + max(out_bytes, 1)], out_bytes, res, work, st)
    assert r == 0, r
    torch.cuda.synchronize()
    results = res.cpu().numpy().view(np.uint8).view(D.BRESULT_DTYPE)[:n]
    rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    return results, big.cpu().numpy(), rec


def verify(results, big, rec, entries, what=""):
    """entries: (dst, out_len, want bytes or None, status, adler or None) per entry.  Every result, every
    byte of an entry that passes, every byte outside the entries (the guards included), the summary."""
    covered = np.zeros(len(big), dtype=bool)
    nfailed, first_bad, total = 0, 0xFFFFFFFF, 0
    for e, (dst, n, want, status, adl) in enumerate(entries):
        r = results[e]
        got = int(r["status"])
        if isinstance(status, (set, frozenset)):
            assert got in status, (what, e, got, status)
        elif status == "nonzero":
            assert got != 0, (what, e)
        else:
            assert got == status, (what, e, got, status)
        if got == 0:
            assert (int(r["format"]), int(r["out_len"]), int(r["reserved"])) == (3, n, 0), (what, e, r)
            if want is not None:
                assert big[GUARD + dst:GUARD + dst + n].tobytes() == want, (what, e)
                assert int(r["check"]) == (zlib.adler32(want) if adl is None else adl), (what, e)
            total += n
        else:
            assert (int(r["out_len"]), int(r["in_used"]), int(r["check"])) == (0, 0, 0), (what, e, r)
            nfailed += 1
            first_bad = min(first_bad, e)
        if 0 <= dst and dst + n <= len(big) - 2 * GUARD:
            covered[GUARD + dst:GUARD + dst + n] = True
    assert (big[~covered] == CANARY).all(), (what, "a byte outside the entries was written")
    assert (rec.nfailed, rec.first_bad, rec.total_out) == (nfailed, first_bad, total), (what, rec.nfailed, rec.first_bad, rec.total_out)


def whole(ix, z, data, what):
    res, big, rec = launch(z, ix.points, ix.adlers, ix.windows)
    ents = [(int(p["out_off"]), int(p["out_len"]), data[int(p["out_off"]):int(p["out_off"]) + int(p["out_len"])], 0, int(a))
            for p, a in zip(ix.points, ix.adlers)]
    verify(res, big, rec, ents, what)
    ext = ((ix.points["end_bit"] + 7) >> 3) - (ix.points["bit"] >> 3)
    assert (res["in_used"] == ext).all(), what
    assert rec.total_out == len(data) and big[GUARD:GUARD + len(data)].tobytes() == data, what


# ---- 1. the whole decode ---------------------------------------------------------------------------

@pytest.mark.parametrize("span", (1, 65536))
@pytest.mark.parametrize("k", range(10))
def test_whole_decode(k, span):
    name, z, fmt, data = I.round_trip_inputs()[k]
    ix = index_of((name, span), z, fmt="raw" if fmt == "raw" else "auto", span=span)
    whole(ix, z, data, f"{name} span {span}")
    out = D.inflate_indexed(torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda(), ix)
    assert out.dtype == torch.uint8 and out.is_cuda and out.cpu().numpy().tobytes() == data


# ---- 2. windows and bit offsets at their edges -----------------------------------------------------

def wlen_stream():
    """(zlib stream, data): points whose windows hold 0, 7, 37 and 32 767 bytes -- blocks of 7, 30 and
    32 730 literals, then a block of matches exactly 32 767 back, the first byte of that window"""
    if "wlen" not in _cache:
        t = I.text()[200_000:200_000 + 32767]
        d, out = C.Deflate(), bytearray()
        for lo, hi in ((0, 7), (7, 37), (37, 32767)):
            toks = list(t[lo:hi])
            I._block(d, toks)
            I._apply(toks, out)
        toks = [(4, 32767), 120, (6, 32767), (258, 32767), 121, (3, 32767)]
        I._block(d, toks, final=True)
        I._apply(toks, out)
        data = bytes(out)
        z = C.zlib_wrap(d.getvalue(), data)
        assert zlib.decompress(z) == data
        _cache["wlen"] = (z, data)
    return _cache["wlen"]


def test_window_edges():
    z, data = I.window_edge_stream()
    ix = index_of("edge1", z, span=1)
    wl = np.minimum(ix.points["out_off"], W)
    assert 0 in wl and W in wl and int((wl == W).sum()) >= 25   # distances of 32 768 and 32 767 across point starts
    whole(ix, z, data, "window edge")
    z, data = wlen_stream()
    ix = index_of("wlen1", z, span=1)
    wl = [int(v) for v in np.minimum(ix.points["out_off"], W)]
    assert wl == [0, 7, 37, 32767] and wl[1] < 16 and wl[2] % 16 and wl[2] > 16
    whole(ix, z, data, "wlen")


def test_bit_offsets_of_the_sync_flush_stream():
    name, z, fmt, data = I.round_trip_inputs()[9]
    ix = index_of((name, 1), z, span=1)
    p = ix.points
    assert set(int(b) & 7 for b in p["bit"]) == set(range(8))
    # behind a sync flush a point begins with the empty stored block, at any bit of its byte
    stored_first = [k for k in range(1, ix.npoints) if int(p["bit"][k]) & 7 and
                    (int.from_bytes(z[int(p["bit"][k]) >> 3:(int(p["bit"][k]) >> 3) + 2], "little") >> (int(p["bit"][k]) & 7)) & 6 == 0]
    assert len(stored_first) >= 300
    assert int((p["end_bit"][:-1] & 7 != 0).sum()) >= 300      # end_bit inside the byte the next point starts in
    assert (int(p["end_bit"][-1]) + 7) >> 3 == len(z) - 4      # the last point ends in the last DEFLATE byte
    assert int(p["out_len"].max()) < 16384                     # no flush before the end
    whole(ix, z, data, name)


def test_a_point_of_several_ring_wraps():
    name, z, fmt, data = I.round_trip_inputs()[3]
    ix = index_of((name, 100_000), z, span=100_000)
    assert int(ix.points["out_len"][:-1].min()) > 96 << 10 and ix.npoints >= 8
    whole(ix, z, data, name)


# ---- 3. selections ---------------------------------------------------------------------------------

def _entries(ix, data, sel, dst):
    out = []
    for k, d in zip(sel, dst):
        o, n = int(ix.points["out_off"][k]), int(ix.points["out_len"][k])
        out.append((int(d), n, data[o:o + n], 0, int(ix.adlers[k])))
    return out


def test_a_permuted_subset_at_every_alignment():
    z, data = I.window_edge_stream()
    ix = index_of("edge1", z, span=1)
    rng = np.random.default_rng(11)
    sel = [int(v) for v in rng.permutation(ix.npoints)[:32]]
    sel[5] = sel[20]   # the same point twice, to two places
    dst, off = [], 0
    for j, k in enumerate(sel):
        off += (j % 16 - off) % 16   # dst % 16 runs through all 16 residues, twice
        dst.append(off)
        off += int(ix.points["out_len"][k])
    assert set(d % 16 for d in dst) == set(range(16))
    res, big, rec = launch(z, ix.points, ix.adlers, ix.windows, sel, dst, off + 3)
    verify(res, big, rec, _entries(ix, data, sel, dst), "subset")


def test_claim_loop_and_ring_reuse():
    """2 560 entries on at most 2 048 workgroups: every workgroup's ring serves entry after entry.  The
    first 2 048 entries are points whose window is full, so whichever of them a workgroup claims first
    fills its ring to the last byte; the last 512 are such points with out_off forged to 0, whose first
    match reaches 32 768 back, before the first byte: -E_HUFDIS.  The grid is at most 2 048 and claims
    go in index order, so a forged entry runs on a ring that a full-window entry (and perhaps forged
    ones, which write nothing) used before it -- unless a workgroup started so late that the others had
    claimed 2 048 entries of some 50 microseconds each before its first claim, which nothing here can
    rule out and which would only make the ring's bytes older, not the required status another.  A
    decoder that let the match read the ring would give status 0 or -E_ZADL32."""
    z, data = I.window_edge_stream()
    ix = index_of("edge1", z, span=1)
    full = [k for k in range(ix.npoints) if int(ix.points["out_off"][k]) >= 40_000]   # the match blocks: a match comes first
    assert len(full) == 30
    points = np.concatenate([ix.points, ix.points[full]])
    forged = {full[j]: ix.npoints + j for j in range(len(full))}
    points["out_off"][ix.npoints:] = 0
    adlers = np.concatenate([ix.adlers, ix.adlers[full]])
    windows = np.concatenate([ix.windows, ix.windows[full]])
    sel, status = [], []
    for e in range(2560):
        k = full[e % len(full)]
        sel.append(k if e < 2048 else forged[k])
        status.append(0 if e < 2048 else E["E_HUFDIS"])
    dst = np.concatenate(([0], np.cumsum(points["out_len"][sel]))).astype(np.int64)
    res, big, rec = launch(z, points, adlers, windows, sel, dst[:-1], int(dst[-1]))
    ents = []
    for e, k in enumerate(sel):
        n = int(points["out_len"][k])
        o = int(ix.points["out_off"][k]) if k < ix.npoints else 0
        ents.append((int(dst[e]), n, data[o:o + n] if status[e] == 0 else None, status[e], None))
        if status[e]:   # the first token failed: nothing of the entry before, or of anything, shows
            assert (big[GUARD + int(dst[e]):GUARD + int(dst[e]) + n] == CANARY).all(), e
    verify(res, big, rec, ents, "2560 entries")
    assert rec.nfailed == 512


# ---- 4. a forged index: the entry alone fails ------------------------------------------------------

def test_index_errors():
    z, data = I.window_edge_stream()
    one = index_of("edge1", z, span=1)         # every block a point: the true boundaries
    ix = index_of("edge3000", z, span=3000)    # two blocks a point
    assert ix.npoints >= 20 and one.npoints > ix.npoints
    k = int(np.searchsorted(ix.points["out_off"], 40_000))   # the first point of match blocks, 32 768 back: its window is full
    p0 = ix.points[k]
    assert 0 < k < ix.npoints - 2 and int(p0["out_off"]) == 40_000 and data[int(p0["out_off"])] == data[int(p0["out_off"]) - W]
    inner = [int(b) for b in one.points["bit"] if int(p0["bit"]) < int(b) < int(p0["end_bit"])]
    assert inner
    total = int(ix.points["out_len"].sum())
    RANGE, SZ, ADL = E["E_RANGE"], E["E_SZ"], E["E_ZADL32"]

    def case(what, status, verify_adler=True, sel=None, dst=None, **forge):
        points, adlers, windows = ix.points.copy(), ix.adlers.copy(), ix.windows.copy()
        for f, v in forge.items():
            if f == "window":
                windows[k, v] ^= 0x20
            elif f == "adler":
                adlers[k] ^= v
            else:
                points[f][k] = v
        s = list(range(ix.npoints)) if sel is None else sel
        d = [int(v) for v in ix.points["out_off"]] if dst is None else dst
        res, big, rec = launch(z, points, adlers if verify_adler else None, windows, s if sel is not None else None,
                               d if dst is not None else None, total)
        ents = _entries(ix, data, range(ix.npoints), d)
        dk, nk = ents[k][0], int(points["out_len"][k])
        ents[k] = (dk, nk, None, status, None)
        verify(res, big, rec, ents, what)

    sel = list(range(ix.npoints))
    sel[k] = ix.npoints
    case("sel >= npoints", RANGE, sel=sel)
    sel[k] = 0xFFFFFFFF
    case("sel = 2^32 - 1", RANGE, sel=sel)
    dst = [int(v) for v in ix.points["out_off"]]
    dst[k] = total - int(p0["out_len"]) + 1
    case("dst outside the output", RANGE, dst=dst)
    dst[k] = (1 << 64) - 8
    case("dst far outside", RANGE, dst=dst)
    case("bit = end_bit", RANGE, bit=int(p0["end_bit"]))
    case("bit > end_bit", RANGE, bit=int(p0["end_bit"]) + 9)
    case("end_bit past the stream", RANGE, end_bit=8 * len(z) + 1)
    case("out_len one too small", SZ, out_len=int(p0["out_len"]) - 1)
    case("out_len one too large", SZ, out_len=int(p0["out_len"]) + 1)
    case("end_bit at an earlier boundary", SZ, end_bit=inner[0])
    case("end_bit at a later boundary", SZ, end_bit=int(ix.points["end_bit"][k + 1]))
    case("a window byte that is referenced", ADL, window=0)
    case("an Adler-32 flipped", ADL, adler=1 << 9)
    case("bit + 1", "nonzero", bit=int(p0["bit"]) + 1)   # a decode error or -E_ZADL32, never status 0
    # without verification a wrong window gives wrong bytes, and status 0
    points, windows = ix.points.copy(), ix.windows.copy()
    windows[k, 0] ^= 0x20
    res, big, rec = launch(z, points, None, windows)
    assert int(res["status"][k]) == 0 and rec.nfailed == 0
    o, n = int(p0["out_off"]), int(p0["out_len"])
    got = big[GUARD:GUARD + total].tobytes()
    assert got[:o] == data[:o] and got[o + n:] == data[o + n:] and got[o] == data[o] ^ 0x20
    assert (big[:GUARD] == CANARY).all() and (big[GUARD + total:] == CANARY).all()


# ---- 5. a damaged stream behind a sound index ------------------------------------------------------

def test_bit_flips_in_the_stream():
    z, data, flips = I.flip_stream()
    ix = index_of("flip1", z, span=1)
    assert ix.npoints >= 8
    L = D.lib()
    n = ix.npoints
    pt, at, wt = ix.cuda()
    zt = torch.zeros(len(z), dtype=torch.uint8, device="cuda")
    res = torch.empty(n * 4, dtype=torch.int64, device="cuda")
    st = torch.empty(2, dtype=torch.int64, device="cuda")
    work = torch.empty(int(L.dmx_inflate_points_work(n)), dtype=torch.uint8, device="cuda")
    big = torch.empty(GUARD + len(data) + GUARD, dtype=torch.uint8, device="cuda")
    want = [data[int(p["out_off"]):int(p["out_off"]) + int(p["out_len"])] for p in ix.points]
    damaged = 0
    for f in flips:
        zt.copy_(torch.frombuffer(bytearray(f), dtype=torch.uint8))
        big.fill_(CANARY)
        res.fill_(-1)
        assert D.inflate_points_async(zt, pt, at, wt, n, None, None, n, big[GUARD:GUARD + len(data)], len(data), res, work, st) == 0
        out = big.cpu().numpy()   # (synchronises: the call returned)
        results = res.cpu().numpy().view(np.uint8).view(D.BRESULT_DTYPE)
        rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
        bad = 0
        for k in range(n):
            o = int(ix.points["out_off"][k])
            if int(results["status"][k]) == 0:
                assert out[GUARD + o:GUARD + o + len(want[k])].tobytes() == want[k]
            else:
                bad += 1
        assert rec.nfailed == bad
        assert (out[:GUARD] == CANARY).all() and (out[GUARD + len(data):] == CANARY).all()
        damaged += bad > 0
    assert damaged >= 150   # (a flip in the trailer, or in a stored block's padding, damages no point)


# ---- 6. range reads --------------------------------------------------------------------------------

def test_range_reads():
    name, z, fmt, data = I.round_trip_inputs()[4]   # level 6, gzip
    ix = index_of((name, 65536), z, span=65536)
    zt = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    n = len(data)
    rng = np.random.default_rng(3)
    po = [int(v) for v in ix.points["out_off"]]
    ranges = [[int(rng.integers(0, n - 6000)), int(rng.integers(0, 6000))] for _ in range(200)]
    ranges += [[po[3] + 10, 500], [po[5] - 1, 2], [po[7] - 5, po[9] - po[7] + 10], [po[2], po[3] - po[2]]]   # inside one point, across two, three, one whole
    ranges += [[0, 0], [n, 0], [12345, 0], [n - 1, 1], [0, 1], [0, 70000], [n - 70000, 70000]]
    out, offsets = D.zindex_read_ranges(zt, ix, ranges)
    offs = offsets.cpu().numpy()
    got = out.cpu().numpy().tobytes()
    assert out.dtype == torch.uint8 and offsets.dtype == torch.int64 and len(offs) == len(ranges) + 1 and offs[-1] == len(got)
    for q, (o, ln) in enumerate(ranges):
        assert offs[q + 1] - offs[q] == ln and got[offs[q]:offs[q + 1]] == data[o:o + ln], (q, o, ln)
    assert D.zindex_pread(zt, ix, po[7] - 5, po[9] - po[7] + 10).cpu().numpy().tobytes() == data[po[7] - 5:po[9] + 5]
    assert D.zindex_pread(zt, ix, n - 1, 1).cpu().numpy().tobytes() == data[-1:]
    assert D.zindex_pread(zt, ix, n, 0).numel() == 0
    assert D.zindex_pread(zt, ix, 0, n, verify=False).cpu().numpy().tobytes() == data
    out, offsets = D.zindex_read_ranges(zt, ix, np.zeros((0, 2), dtype=np.int64))
    assert out.numel() == 0 and offsets.cpu().tolist() == [0]
    for bad in ([n, 1], [n - 3, 4], [n + 1, 0], [-1, 2], [5, -1]):
        with pytest.raises(ValueError):
            D.zindex_pread(zt, ix, *bad)
    # a damaged stream under a range read: the status of the point that fails
    zb = bytearray(z)
    zb[int(ix.points["bit"][4]) // 8 + 200] ^= 4
    with pytest.raises(D.DeflateError):
        D.zindex_pread(torch.frombuffer(zb, dtype=torch.uint8).cuda(), ix, po[4] + 100, 50)
    assert D.zindex_pread(torch.frombuffer(zb, dtype=torch.uint8).cuda(), ix, po[6], 50).cpu().numpy().tobytes() == data[po[6]:po[6] + 50]


# ---- 7. in a graph ---------------------------------------------------------------------------------

def test_points_in_a_graph():
    """the call captured once on a side stream -- two kernels, one after the other -- and replayed
    after the compressed bytes and the index tensors were overwritten in place with another stream's"""
    L = D.lib()
    streams = []
    for seed in (1, 2, 3):
        data = D.gen_text(30_000, 40 + seed).tobytes()
        z = I.deflate(data, 6, 15, flush_every=3000)
        streams.append((z, data, D.zindex_build(z, span=1)))
    n = streams[0][2].npoints
    assert n >= 10 and all(s[2].npoints == n for s in streams)
    zcap = max(len(s[0]) for s in streams)
    zt = torch.zeros(zcap, dtype=torch.uint8, device="cuda")
    pt = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    at = torch.zeros(n, dtype=torch.int32, device="cuda")
    wt = torch.zeros((n, W), dtype=torch.uint8, device="cuda")
    res = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    big = torch.zeros(GUARD + 30_000 + GUARD, dtype=torch.uint8, device="cuda")
    work = torch.empty(int(L.dmx_inflate_points_work(n)), dtype=torch.uint8, device="cuda")

    def set_input(z, ix):
        zt.zero_()
        zt[:len(z)].copy_(torch.frombuffer(bytearray(z), dtype=torch.uint8))
        pt.copy_(torch.from_numpy(ix.points.view("<i8").reshape(n, 4).copy()))
        at.copy_(torch.from_numpy(ix.adlers.view(np.int32).copy()))
        wt.copy_(torch.from_numpy(ix.windows))

    def enqueue():
        return D.inflate_points_async(zt, pt, at, wt, n, None, None, n, big[GUARD:GUARD + 30_000], 30_000, res, work, st)

    set_input(streams[0][0], streams[0][2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the kernels are loaded before the capture
        assert enqueue() == 0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r = enqueue()
    assert r == 0
    for z, data, ix in (streams[1], streams[2], streams[0]):
        set_input(z, ix)
        big.fill_(CANARY)
        res.fill_(-1)
        st.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        results = res.cpu().numpy().view(np.uint8).view(D.BRESULT_DTYPE)
        rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
        ents = _entries(ix, data, range(n), ix.points["out_off"])
        verify(results, big.cpu().numpy(), rec, ents, "replay")
        assert rec.total_out == 30_000
