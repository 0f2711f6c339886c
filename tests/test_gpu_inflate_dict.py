"""Batches of streams with preset dictionaries on the GPU (dmx_inflate_batch_dict_async,
csrc/dmx_inflate_dev.hip): zlib streams with FDICT and raw streams primed from dictionaries of every
length and alignment, crafted first tokens that reach the dictionary's ends, rings that are reused by
one stream after the other, the measure pass, a captured call, and the old entry on the old inputs.
zlib.decompressobj(wbits, zdict=d) is the reference for bytes (inflate_dict_inputs.Case); the contract
in include/dmx.h names the statuses.  Every case is one or a few launches on streams of at most 100 KB.
"""
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
import deflate_craft as C
import inflate_dict_inputs as I

pytestmark = pytest.mark.gpu

E = I.E
ZLIB, GZIP, RAW, AUTO, MEASURE = I.ZLIB, I.GZIP, I.RAW, I.AUTO, D.DMX_BATCH_MEASURE
NODICT = D.DMX_BATCH_NODICT
CANARY = 0xA5
GUARD = 64
NOLIMIT = (1 << 64) - 1


class Dicts:
    """the dictionary buffer of a call: every distinct dictionary once, at an address whose low four
    bits are `align` (CUDA allocations are 256-byte aligned), with other bytes between them"""

    def __init__(self, align=0):
        self.align, self.buf, self.recs, self.index = align, bytearray(), [], {}

    def add(self, d):
        if d is None:
            return NODICT
        if d not in self.index:
            while len(self.buf) % 16 != self.align:
                self.buf.append(0x5A)
            self.index[d] = len(self.recs)
            self.recs.append((len(self.buf), len(d)))
            self.buf += d
        return self.index[d]


def _launch(cases, flags, first=GUARD, align=0, out=True, caps=None, dict_of=None, recs=None):
    """One call on fresh buffers.  The streams are packed with no padding, the windows lie back to back
    from out_off `first`; returns (results, out bytes or None, BatchStatus, desc)."""
    L = D.lib()
    n = len(cases)
    dd = Dicts(align)
    of = np.array([dd.add(c.d) for c in cases], dtype=np.uint32)
    if dict_of is not None:
        of = np.array(dict_of, dtype=np.uint32)
    recs = dd.recs if recs is None else recs
    desc = np.zeros((n, 4), dtype=np.uint64)
    zoff, ooff = 0, first
    for k, c in enumerate(cases):
        cap = (len(c.want) if c.want is not None else 0) if caps is None else caps[k]
        desc[k] = (zoff, len(c.z), 0 if cap == NOLIMIT else ooff, cap)
        zoff += len(c.z)
        ooff += 0 if cap == NOLIMIT else cap
    out_bytes = ooff + GUARD
    z = b"".join(c.z for c in cases)
    zt = torch.frombuffer(bytearray(z or b"\0"), dtype=torch.uint8).cuda()[:len(z)]
    dt = torch.from_numpy(desc.view(np.int64).copy()).cuda()
    dbuf = torch.frombuffer(bytearray(bytes(dd.buf) or b"\0"), dtype=torch.uint8).cuda()[:len(dd.buf)]
    nd = len(recs)
    dicts_t = torch.from_numpy(np.array(recs, dtype=np.uint64).reshape(-1, 2).view(np.int64).copy()).cuda()
    of_t = torch.from_numpy(of.view(np.int32).copy()).cuda()
    res = torch.full((max(n, 1) * 4,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(int(L.dmx_inflate_batch_dict_work(n, nd)), dtype=torch.uint8, device="cuda")
    ot = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device="cuda") if out else None
    r = D.inflate_batch_dict_async(zt, dt, n, flags, dbuf, dicts_t, nd, of_t, ot, out_bytes if out else 0, res, work, st)
    assert r == 0, r
    torch.cuda.synchronize()
    results = res.cpu().numpy().view(np.uint8).view(D.BRESULT_DTYPE)[:n]
    rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    return results, (ot.cpu().numpy() if out else None), rec, desc


def _check(c):
    return {ZLIB: zlib.adler32, GZIP: zlib.crc32}.get(c.fmt, lambda d: 0)(c.want)


def _verify(cases, desc, results, out, rec, what="", statuses=None, stored=True):
    """every result, every decoded byte, every byte outside the windows, and the summary"""
    bad = []
    covered = np.zeros(len(out), dtype=bool) if out is not None else None
    nfailed, first_bad, total = 0, 0xFFFFFFFF, 0
    for k, c in enumerate(cases):
        r = results[k]
        want = c.status if statuses is None else statuses[k]
        got = (int(r["status"]), int(r["out_len"]), int(r["in_used"]), int(r["check"]), int(r["reserved"]))
        off, cap = int(desc[k][2]), int(desc[k][3])
        if want:
            nfailed += 1
            first_bad = min(first_bad, k)
            if got != (want, 0, 0, 0, 0):
                bad.append((what, k, c.name, got, want))
        else:
            n = len(c.want)
            total += n
            if got != (0, n, c.used, _check(c), 0) or int(r["format"]) != c.fmt:
                bad.append((what, k, c.name, got, int(r["format"]), (0, n, c.used, _check(c), 0), c.fmt))
            elif out is not None and stored and out[off:off + n].tobytes() != c.want:
                bad.append((what, k, c.name, "bytes differ"))
        if out is not None and stored and want != E["E_RANGE"] and cap != NOLIMIT:
            covered[off:off + cap] = True
    assert not bad, bad[:10]
    assert (rec.nfailed, rec.first_bad, rec.total_out) == (nfailed, first_bad, total), what
    if out is not None:
        assert (out[~covered] == CANARY).all(), what + ": a byte outside the windows was written"


# ---- 1. every dictionary length, at buffer offsets 0, 1 and 3, windows from out_off 0 and 5 ---------

@pytest.mark.parametrize("align", [0, 1, 3])
def test_dictionary_lengths(align):
    cases = I.written_cases()
    assert sorted({len(c.d) for c in cases}) == I.DLENS
    for first in (0, 5):
        # the two framings need their own flags: zlib streams under AUTO, raw streams under RAW
        for fmt, flags in ((ZLIB, AUTO), (RAW, RAW)):
            sub = [c for c in cases if c.fmt == fmt]
            results, out, rec, desc = _launch(sub, flags, first=first, align=align)
            _verify(sub, desc, results, out, rec, what=f"align {align} out_off {first} fmt {fmt}")


# ---- 2. crafted first tokens ------------------------------------------------------------------------

def test_crafted_first_tokens():
    cases = I.crafted_cases()
    names = " ".join(c.name for c in cases)
    for part in ("first primed byte dlen 32768", "distance 1", "distance 3", "too far", "across a stored block"):
        assert part in names
    for fmt, flags in ((ZLIB, ZLIB), (RAW, RAW)):
        sub = [c for c in cases if c.fmt == fmt]
        for first in (0, 5):
            results, out, rec, desc = _launch(sub, flags, first=first, align=3)
            _verify(sub, desc, results, out, rec, what=f"crafted fmt {fmt} out_off {first}")


# ---- 3. 100 KiB against a 32 KiB dictionary ---------------------------------------------------------

def test_long_streams_wrap_the_ring():
    d = D.gen_text(32768, 77).tobytes()
    text = D.gen_text(100 * 1024, 78).tobytes()
    a = I.Case("100 KiB text", I.deflate(text, d, 15), ZLIB, d)
    assert a.z[1] & 0x20 and a.want == text
    # 70 000 stored bytes, then a match at distance 32 768 at output position 70 000, then a tail
    body = D.gen_random(70000, 5).tobytes()
    w = C.Deflate().stored(body[:65535], False).stored(body[65535:], False)
    w.fixed_block(C.match(258, 32768) + C.lits(b"tail") + [("L", 256)], False)
    w.stored(D.gen_text(30000, 6).tobytes(), True)
    says = I.zlib_says(w.getvalue(), d, -15)
    b = I.Case("distance 32768 at 70000", I.fdict_wrap(w.getvalue(), d, says[0]), ZLIB, d)
    assert b.want[70000:70258] == body[70000 - 32768:70258 - 32768] and len(b.want) == 100262
    cases = [a, b, a]
    results, out, rec, desc = _launch(cases, ZLIB, first=3, align=1)
    _verify(cases, desc, results, out, rec, what="long")


# ---- 4. negative cases in a mixed batch -------------------------------------------------------------

def _neighbours():
    d = I.dictionary(258)
    data = I.payload(d, 9)
    return [I.Case("neighbour fdict", I.deflate(data, d, 15), ZLIB, d), I.Case("neighbour plain", I.deflate(data, None, 15), ZLIB, None)]


def test_negative_cases_leave_neighbours_intact():
    neg = [c for c in I.negative_cases() if c.fmt != RAW]
    nb = _neighbours()
    cases = []
    for k, c in enumerate(neg):
        cases += [nb[k % 2], c]
    cases.append(nb[0])
    results, out, rec, desc = _launch(cases, AUTO, align=1)
    _verify(cases, desc, results, out, rec, what="negative")
    byname = {c.name: k for k, c in enumerate(cases)}
    # the no-FDICT stream and the gzip member equal the decode without any dictionary
    for name in ("no fdict, a dictionary given", "gzip under auto, a dictionary given"):
        c = cases[byname[name]]
        plain = I.Case(name, c.z, c.fmt, None)
        r2, o2, _, d2 = _launch([plain], AUTO)
        k = byname[name]
        assert results[k].tobytes() == r2[0].tobytes()
        n = len(c.want)
        assert out[int(desc[k][2]):int(desc[k][2]) + n].tobytes() == o2[int(d2[0][2]):int(d2[0][2]) + n].tobytes() == c.want


def test_descriptor_errors_are_per_stream():
    nb = _neighbours()
    d = nb[0].d
    cases = [nb[0], nb[0], nb[1], nb[0], nb[0], nb[1]]
    dd = Dicts(0)
    dd.add(d)
    off, n = dd.recs[0]
    # dictionary 1 ends one byte past dict_bytes, dictionary 2 begins past it, dictionary 3 has a length that wraps
    recs = [(off, n), (off + 1, n), (off + n + 1, 0), (1, NOLIMIT)]
    dict_of = [0, 4, 4, 1, 2, 3]     # 4: no such dictionary (ndicts == 4)
    statuses = [0, E["E_RANGE"], E["E_RANGE"], E["E_RANGE"], E["E_RANGE"], E["E_RANGE"]]
    results, out, rec, desc = _launch(cases, AUTO, dict_of=dict_of, recs=recs)
    _verify(cases, desc, results, out, rec, what="descriptor", statuses=statuses)
    assert [int(r["format"]) for r in results] == [ZLIB, 0, 0, 0, 0, 0]
    # a stream with NODICT beside them is no error, and neither is an index that nobody uses
    results, out, rec, desc = _launch(cases[:3], AUTO, dict_of=[0, 0, NODICT], recs=recs)
    _verify(cases[:3], desc, results, out, rec, what="unused bad records")


# ---- 5. one ring after the other --------------------------------------------------------------------

def test_ring_reuse_never_reads_the_previous_dictionary():
    n = 2560   # more than the grid's fixed bound of 2 048: some workgroup decodes several streams in a row
    ds = [I.dictionary(17), I.dictionary(4097), I.dictionary(32768)]
    kinds = []
    for q, d in enumerate(ds):
        raw = C.Deflate().fixed_block(C.match(30, 1) + C.match(31, min(len(d), 32768)) + C.lits(b"%03d" % q) + [("L", 256)], True).getvalue()
        kinds.append(I.Case(f"ring dict {q}", raw, RAW, d))
        assert len(kinds[-1].want) == 64
    kinds.append(I.Case("ring no dictionary", I.raw_match(61, 1), RAW, None, E["E_HUFDIS"]))
    cases = [kinds[k % 4] for k in range(n)]
    results, out, rec, desc = _launch(cases, RAW, align=3)
    _verify(cases, desc, results, out, rec, what="ring")
    assert rec.nfailed == n // 4


# ---- 6. the measure pass ----------------------------------------------------------------------------

def test_measure_equals_the_storing_pass():
    nb = _neighbours()
    cases = [c for c in I.written_cases() if c.fmt == ZLIB] + [c for c in I.crafted_cases() if c.fmt == ZLIB]
    cases += [c for c in I.negative_cases() if c.fmt != RAW] + nb
    stored = _launch(cases, AUTO, align=1)
    _verify(cases, stored[3], stored[0], stored[1], stored[2], what="storing")
    measured = _launch(cases, AUTO | MEASURE, align=1, out=False, caps=[NOLIMIT] * len(cases))
    _verify(cases, measured[3], measured[0], None, measured[2], what="measure (NULL)")
    for f in ("status", "format", "out_len", "in_used", "check"):
        assert (stored[0][f] == measured[0][f]).all(), f
    again = _launch(cases, AUTO | MEASURE, align=1)
    _verify(cases, again[3], again[0], None, again[2], what="measure")
    assert (again[1] == CANARY).all(), "the measure pass wrote"
    raws = [c for c in I.written_cases() + I.crafted_cases() if c.fmt == RAW]
    m = _launch(raws, RAW | MEASURE, out=False, caps=[NOLIMIT] * len(raws))
    _verify(raws, m[3], m[0], None, m[2], what="measure raw")


# ---- 7. a captured call ------------------------------------------------------------------------------

def test_dictionary_adler_is_in_the_graph():
    """reset, Adler, decode captured once and replayed twice; between the replays the dictionary's
    bytes change in place, and the streams that named the old bytes become -E_ZPDICT"""
    L = D.lib()
    d = I.dictionary(300)
    data = I.payload(d, 3)
    cases = [I.Case("g fdict", I.deflate(data, d, 15), ZLIB, d), I.Case("g plain", I.deflate(data, None, 15), ZLIB, None),
             I.Case("g fdict", I.deflate(data[:700], d, 15), ZLIB, d), I.Case("g gzip", I.deflate(data, None, 31), GZIP, None)]
    n, wcap = len(cases), 4096
    z = b"".join(c.z for c in cases)
    desc = np.zeros((n, 4), dtype=np.int64)
    off = 0
    for k, c in enumerate(cases):
        desc[k] = (off, len(c.z), GUARD + k * wcap, wcap)
        off += len(c.z)
    zt = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    dt = torch.from_numpy(desc).cuda()
    dbuf = torch.frombuffer(bytearray(b"\x5a" + d), dtype=torch.uint8).cuda()
    dicts_t = torch.from_numpy(np.array([[1, len(d)]], dtype=np.int64)).cuda()
    of_t = torch.from_numpy(np.array([0, NODICT, 0, 0], dtype=np.uint32).view(np.int32).copy()).cuda()
    res = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.zeros(GUARD + n * wcap + GUARD, dtype=torch.uint8, device="cuda")
    work = torch.empty(int(L.dmx_inflate_batch_dict_work(n, 1)), dtype=torch.uint8, device="cuda")

    def enqueue():
        return D.inflate_batch_dict_async(zt, dt, n, AUTO, dbuf, dicts_t, 1, of_t, out, out.numel(), res, work, st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the kernels are loaded before the capture
        assert enqueue() == 0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r = enqueue()
    assert r == 0
    for replay, statuses in ((0, [0, 0, 0, 0]), (1, [E["E_ZPDICT"], 0, E["E_ZPDICT"], 0])):
        if replay:
            dbuf[1 + 100] ^= 1   # one byte of the dictionary, in place
        out.fill_(CANARY)
        res.fill_(-1)
        st.fill_(-1)
        work.fill_(0xEE)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        results = res.cpu().numpy().view(np.uint8).view(D.BRESULT_DTYPE)
        rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
        _verify(cases, desc.astype(np.uint64), results, out.cpu().numpy(), rec, what=f"replay {replay}", statuses=statuses)


# ---- 8. the old entry on the old inputs ---------------------------------------------------------------

def test_old_entry_equals_the_new_without_dictionaries():
    L = D.lib()
    datas = [D.gen_text(5000 + 777 * k, k).tobytes() for k in range(5)]
    zs = [I.deflate(datas[0], None, 15), I.deflate(datas[1], None, 31), I.deflate(datas[2], None, 15)[:-3],
          I.deflate(datas[3], I.dictionary(300), 15), I.deflate(datas[4], None, 15, level=0)]
    z = b"".join(zs)
    n, wcap = len(zs), 8192
    desc = np.zeros((n, 4), dtype=np.int64)
    off = 0
    for k, s in enumerate(zs):
        desc[k] = (off, len(s), GUARD + k * wcap, wcap)
        off += len(s)
    zt = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    dt = torch.from_numpy(desc).cuda()
    got = []
    for new in (False, True, True):
        res = torch.full((n * 4,), -1, dtype=torch.int64, device="cuda")
        st = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((GUARD + n * wcap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        work = torch.empty(int(L.dmx_inflate_batch_work(n)), dtype=torch.uint8, device="cuda")
        if new:
            of_t = torch.full((n,), -1, dtype=torch.int32, device="cuda") if len(got) == 2 else None
            r = D.inflate_batch_dict_async(zt, dt, n, AUTO, None, None, 0, of_t, out, out.numel(), res, work, st)
        else:
            r = D.inflate_batch_async(zt, dt, n, AUTO, out, out.numel(), res, work, st)
        assert r == 0
        torch.cuda.synchronize()
        got.append((res.cpu().numpy().tobytes(), st.cpu().numpy().tobytes(), out.cpu().numpy().tobytes()))
    assert got[0] == got[1] == got[2]
    results = np.frombuffer(got[0][0], dtype=D.BRESULT_DTYPE)
    assert [int(s) for s in results["status"]] == [0, 0, E["E_ZADL32"], E["E_ZPDICT"], 0]
    # and through the convenience call: zdict=None is the old entry, an FDICT stream decodes with zdict
    d = I.dictionary(300)
    o, offs, r = D.inflate_batch([zs[3], zs[0]], zdict=d)
    assert o.cpu().numpy().tobytes() == datas[3] + datas[0] and [int(x) for x in r["in_used"]] == [len(zs[3]), len(zs[0])]
    o, offs, r = D.inflate_batch([zs[3], zs[0]], zdict=[b"x", d], dict_of=[1, None], sizes=[len(datas[3]), len(datas[0])])
    assert o.cpu().numpy().tobytes() == datas[3] + datas[0]
    with pytest.raises(D.DeflateError) as ei:
        D.inflate_batch([zs[0], zs[3]])
    assert ei.value.code == E["E_ZPDICT"]
