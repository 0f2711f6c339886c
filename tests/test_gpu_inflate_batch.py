"""Batches of independent streams on the GPU (dmx_inflate_batch_async, csrc/dmx_inflate_dev.hip and
the CRC pass of csrc/dmx_crc.hip): zlib streams, gzip members and raw DEFLATE streams side by side,
each with a result of its own.  Python's zlib is the reference for bytes, the host decoder
(D.deflate_decompress) and the corpus' status table (deflate_craft.STATUS) for statuses.  Every case
is one or a few launches on streams of at most about 200 KB.
"""
import struct
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
import deflate_craft as C
from test_inflate_conformance import _host, flipped_streams, truncation_status

pytestmark = pytest.mark.gpu

E = {k: -v for k, v in D.E.items()}
ZLIB, GZIP, RAW, MEASURE = D.DMX_BATCH_ZLIB, D.DMX_BATCH_GZIP, D.DMX_BATCH_RAW, D.DMX_BATCH_MEASURE
CANARY = 0xA5
GUARD = 64          # canary bytes in front of the first window and behind the last
NOLIMIT = (1 << 64) - 1
LENGTHS = [0, 1, 15, 16, 17, 16383, 16384, 16385, 32767, 32768, 32769, 65537, 200_003]


class Ent:
    """One stream of a batch: its bytes (junk behind them included), its framing, what it decodes to
    (None: it fails with `status`) and its window's capacity (the decoded length unless given)."""

    def __init__(self, z, fmt, want=None, status=0, junk=0, cap=None, mstatus=None, window=True, mwant=None):
        self.z, self.fmt, self.want, self.status, self.junk = z, fmt, want, status, junk
        self.mwant = mwant     # what the measure pass sees where it passes a stream the decode refuses
        self.cap = cap if cap is not None else (len(want) if want is not None else 0)
        self.mstatus = status if mstatus is None else mstatus   # under DMX_BATCH_MEASURE
        self.window = window   # False: the test places this entry's descriptor itself

    def check(self):
        return {ZLIB: zlib.adler32, GZIP: zlib.crc32}.get(self.fmt, lambda d: 0)(self.want)


def _payload(kind, n, seed):
    if kind == 0:
        return D.gen_text(n, seed).tobytes()
    if kind == 1:
        return D.gen_random(n, seed).tobytes()
    return bytes(n)


def _deflate(data, level=6, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits)
    return c.compress(data) + c.flush()


def _layout(ents):
    """(z, desc): the streams packed with no padding, the windows back to back behind GUARD canaries"""
    desc = np.zeros((len(ents), 4), dtype=np.uint64)
    zoff, ooff = 0, GUARD
    for k, e in enumerate(ents):
        desc[k] = (zoff, len(e.z), ooff, e.cap)
        zoff += len(e.z)
        ooff += e.cap
    return b"".join(e.z for e in ents), desc, ooff + GUARD


def _launch(z, desc, flags, out_bytes, out=True):
    """One call on fresh buffers: (results, out bytes or None, BatchStatus); the records start poisoned"""
    n = len(desc)
    L = D.lib()
    zt = torch.frombuffer(bytearray(z or b"\0"), dtype=torch.uint8).cuda()
    dt = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.uint64).view(np.int64).reshape(-1, 4).copy()).cuda()
    res = torch.full((max(n, 1) * 4,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(int(L.dmx_inflate_batch_work(n)), dtype=torch.uint8, device="cuda")
    ot = torch.full((max(out_bytes, 1),), CANARY, dtype=torch.uint8, device="cuda") if out else None
    r = D.inflate_batch_async(zt[:len(z)], dt, n, flags, ot, out_bytes if out else 0, res, work, st)
    assert r == 0, r
    torch.cuda.synchronize()
    results = res.cpu().numpy().view(np.uint8).view(D.BRESULT_DTYPE)[:n]
    rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    return results, (ot.cpu().numpy() if out else None), rec


def _verify(ents, desc, results, out, rec, measure=False, what=""):
    """every result, every decoded byte, every byte outside the windows, and the summary"""
    bad = []
    covered = np.zeros(len(out), dtype=bool) if out is not None else None
    nfailed, first_bad, total = 0, 0xFFFFFFFF, 0
    for k, e in enumerate(ents):
        r = results[k]
        want = e.mstatus if measure else e.status
        got = (int(r["status"]), int(r["out_len"]), int(r["in_used"]), int(r["check"]), int(r["reserved"]))
        if want:
            nfailed += 1
            first_bad = min(first_bad, k)
            if got != (want, 0, 0, 0, 0):
                bad.append((what, k, got, want))
        else:
            n = len(e.want)
            total += n
            if got != (0, n, len(e.z) - e.junk, e.check(), 0) or int(r["format"]) != e.fmt:
                bad.append((what, k, got, int(r["format"]), (0, n, len(e.z) - e.junk, e.check(), 0), e.fmt))
            elif not measure:
                off = int(desc[k][2])
                if out[off:off + n].tobytes() != e.want:
                    bad.append((what, k, "bytes differ"))
        if out is not None and not measure and e.window and want != E["E_RANGE"]:
            covered[int(desc[k][2]):int(desc[k][2]) + int(desc[k][3])] = True
    assert not bad, bad[:10]
    assert (rec.nfailed, rec.first_bad, rec.total_out) == (nfailed, first_bad, total), what
    if out is not None:
        assert (out[~covered] == CANARY).all(), what + ": a byte outside the windows was written"


def _run(ents, flags, what=""):
    z, desc, out_bytes = _layout(ents)
    results, out, rec = _launch(z, desc, flags, out_bytes)
    _verify(ents, desc, results, out, rec, what=what)


def _run_measure(ents, desc_z, flags, what=""):
    """DMX_BATCH_MEASURE with d_out NULL, and with an output that must stay untouched"""
    z, desc, out_bytes = desc_z
    results, _, rec = _launch(z, desc, flags | MEASURE, out_bytes, out=False)
    _verify(ents, desc, results, None, rec, measure=True, what=what + " (NULL)")
    results, out, rec = _launch(z, desc, flags | MEASURE, out_bytes)
    _verify(ents, desc, results, None, rec, measure=True, what=what)
    assert (out == CANARY).all(), what + ": the measure pass wrote"


# ---- 1. the mixed batch --------------------------------------------------------------------

CODECS = [(ZLIB, 0, 15), (ZLIB, 1, 15), (ZLIB, 6, 15), (ZLIB, 9, 15), (GZIP, 6, 31), (RAW, 6, -15)]
_mixed_cache = {}


def _mixed():
    """every length x every codec, the payload kinds by turns; 1..7 bytes of junk behind every third"""
    if not _mixed_cache:
        ents = []
        for i, n in enumerate(LENGTHS):
            for j, (fmt, level, wbits) in enumerate(CODECS):
                data = _payload((i + j) % 3, n, 100 + i)
                junk = (1 + (i + j) % 7) if (i * len(CODECS) + j) % 3 == 0 else 0
                ents.append(Ent(_deflate(data, level, wbits) + bytes([0x5A] * junk), fmt, data, junk=junk))
        _mixed_cache["all"] = ents
    return _mixed_cache["all"]


def test_mixed_batch():
    ents = _mixed()
    assert len(ents) == 78
    auto = [e for e in ents if e.fmt != RAW]
    _run(auto, D.DMX_BATCH_AUTO, "auto")
    for fmt in (ZLIB, GZIP, RAW):
        _run([e for e in ents if e.fmt == fmt], fmt, f"explicit {fmt}")
    # the same members under the wrong explicit framing: every one fails, and alone
    z, desc, out_bytes = _layout([e for e in ents if e.fmt == GZIP])
    r, _, rec = _launch(z, desc, ZLIB, out_bytes)
    assert (r["status"] == E["E_ZCMPMT"]).all() and rec.nfailed == len(r) and rec.first_bad == 0
    z, desc, out_bytes = _layout([e for e in ents if e.fmt == ZLIB])
    r, _, rec = _launch(z, desc, GZIP, out_bytes)
    assert (r["status"] == E["E_ZHEAD"]).all() and rec.total_out == 0


# ---- 2. alignment --------------------------------------------------------------------------

def test_every_input_and_output_alignment():
    data = _payload(0, 70_000, 7)
    zs = {ZLIB: _deflate(data, 6, 15), GZIP: _deflate(data, 6, 31)}
    ents, desc, z = [], np.zeros((256, 4), dtype=np.uint64), bytearray()
    ooff = GUARD
    for k in range(256):
        a, b = k % 16, k // 16
        e = Ent(zs[GZIP if (a + b) % 2 else ZLIB], GZIP if (a + b) % 2 else ZLIB, data)
        z += bytes([0xC3] * ((a - len(z)) % 16))
        ooff += (b - ooff) % 16
        desc[k] = (len(z), len(e.z), ooff, e.cap)
        z += e.z
        ooff += e.cap + 16   # a gap of canaries between the windows
        ents.append(e)
    assert sorted({(int(d[0]) % 16, int(d[2]) % 16) for d in desc}) == [(a, b) for a in range(16) for b in range(16)]
    results, out, rec = _launch(bytes(z), desc, D.DMX_BATCH_AUTO, ooff + GUARD)
    _verify(ents, desc, results, out, rec)


# ---- 3. the window's edge ------------------------------------------------------------------

def test_window_edge():
    ents = [Ent(C.zstream(n), ZLIB, C.expected(n)) for n in C.TWO_BLOCK]
    assert [len(e.want) > 32768 for e in ents] == [True] * 3
    noise = _payload(1, 32768, 3)
    data = noise + noise[:300]   # the only long repeat lies exactly 32 768 back
    ents.append(Ent(_deflate(data, 9, 15), ZLIB, data))
    ents.append(Ent(_deflate(data, 9, -15), RAW, data))
    _run(ents[:4], ZLIB)
    _run([Ent(C.zstream(n)[2:-4], RAW, C.expected(n)) for n in C.TWO_BLOCK] + ents[4:], RAW)


# ---- 4. the conformance corpus -------------------------------------------------------------

CAP = 1 << 20   # more than a stream of a few hundred bytes decodes to, so -E_SZ never hides a status


def _corpus(raw):
    ents = []
    for name, rawz, kind in C.CASES:
        if raw and name == "wrong_adler32":   # zlib-only
            continue
        z = rawz if raw else C.zstream(name)
        fmt = RAW if raw else ZLIB
        if kind == "valid":
            junk = len(z) - (len(rawz) + 6) if name in C.WRAPPED and not raw else 0
            ents.append(Ent(z, fmt, C.expected(name), junk=junk))
        else:
            status = E[C.STATUS[name]]
            if not raw:
                assert _host(z)[1] == status, name
            ents.append(Ent(z, fmt, None, status, cap=CAP))
    return ents


@pytest.mark.parametrize("raw", [False, True])
def test_conformance_corpus(raw):
    ents = _corpus(raw)
    assert sum(e.status == 0 for e in ents) >= 27 and sum(e.status != 0 for e in ents) >= 29
    _run(ents, RAW if raw else ZLIB)
    if not raw:
        _run(ents, D.DMX_BATCH_AUTO, "auto")


# ---- 5. truncation ---------------------------------------------------------------------------

def _gz_member(data, flg=0, extra=b"", name=b"", comment=b"", cm=8, crc=None, isize=None, level=6):
    h = bytes([0x1F, 0x8B, cm, flg]) + struct.pack("<IBB", 0x5F5E100, 2, 3)
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name + b"\0"
    if flg & 16:
        h += comment + b"\0"
    if flg & 2:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + _deflate(data, level, -15) + struct.pack("<II", zlib.crc32(data) if crc is None else crc,
                                                        len(data) if isize is None else isize)


def _prefixes(z, data, fmt):
    """every prefix 1..len-1 of z as an entry of its own over the same in_off, then z itself"""
    n = len(z)
    desc = np.zeros((n, 4), dtype=np.uint64)
    ents = []
    for k in range(1, n + 1):
        desc[k - 1] = (0, k, GUARD + 256 * (k - 1), 256)
        st = _host(z[:k])[1]
        ents.append(Ent(z[:k], fmt, None if st else data, st, cap=256))
    return ents, desc


@pytest.mark.parametrize("which", ["fixed", "dynamic", "stored", "gzip"])
def test_truncation_sweep(which):
    if which == "gzip":
        data = C.sweep_streams()["dynamic"][1]
        z = _gz_member(data, 0x1E, b"\x01\x02\x00\x04", b"name.txt", b"a comment")
        fmt = GZIP
    else:
        z, data = C.sweep_streams()[which]
        fmt = ZLIB
    assert len(data) <= 256
    ents, desc = _prefixes(z, data, fmt)
    assert [e.status for e in ents].count(0) == 1 and ents[-1].status == 0
    if fmt == ZLIB:
        assert [e.status for e in ents[:-1]] == [truncation_status(z, k) for k in range(1, len(z))]
    else:
        assert {e.status for e in ents[:-1]} == {E["E_ZHEAD"], E["E_LEN"], E["E_CRC"]}
    for flags in (D.DMX_BATCH_AUTO, fmt):
        results, out, rec = _launch(z, desc, flags, GUARD + 256 * len(z) + GUARD)
        _verify(ents, desc, results, out, rec, what=which)


# ---- 6. bit flips ----------------------------------------------------------------------------

def test_bitflip_sweep():
    z, data, flips = flipped_streams()
    assert len(flips) == 200
    ents = []
    for c in flips:
        got, st = _host(c)
        ents.append(Ent(c, ZLIB, got, st, cap=None if st == 0 else 1 << 19))   # (2 bits a match at least: < 300 KB)
    assert 0 < sum(e.status == 0 for e in ents) < 200
    _run(ents, ZLIB)


# ---- 7. gzip headers ---------------------------------------------------------------------------

def _gzip_cases():
    data = _payload(0, 5000, 11)
    ents = []
    for flg in range(0, 32, 2):   # all 16 combinations of FHCRC 2, FEXTRA 4, FNAME 8, FCOMMENT 16
        z = _gz_member(data, flg, bytes(range(flg + 3)), b"n" * flg, b"some comment")
        ents.append(Ent(z, GZIP, data))
    ents.append(Ent(_gz_member(data, 0x20), GZIP, None, E["E_RESERV"], cap=8192))
    ents.append(Ent(_gz_member(data, 0x88), GZIP, None, E["E_RESERV"], cap=8192))
    ents.append(Ent(_gz_member(data, 0, cm=7), GZIP, None, E["E_ZCMPMT"], cap=8192))
    ents.append(Ent(_gz_member(data, 8, name=b"x", crc=zlib.crc32(data) ^ 0x100), GZIP, None, E["E_CRC"], cap=8192, mstatus=0,
                    mwant=data))
    ents.append(Ent(_gz_member(data, 0, isize=len(data) + 1), GZIP, None, E["E_LEN"], cap=8192))
    ents.append(Ent(_gz_member(data, 0, crc=1, isize=len(data) + 1), GZIP, None, E["E_CRC"], cap=8192, mstatus=E["E_LEN"]))
    whole = _gz_member(data, 4, b"abcd")
    for cut in range(1, 9):   # the trailer cut at each of its 8 bytes
        ents.append(Ent(whole[:-cut], GZIP, None, E["E_CRC"], cap=8192))
    ents.append(Ent(whole[:14], GZIP, None, E["E_ZHEAD"], cap=8192))       # inside FEXTRA
    for e in ents:
        got, st = _host(e.z)
        assert st == e.status and (st != 0 or got == e.want)
    return ents


def test_gzip_headers():
    ents = _gzip_cases()
    assert len(ents) == 16 + 6 + 8 + 1
    _run(ents, GZIP)
    _run(ents, D.DMX_BATCH_AUTO, "auto")


# ---- 8. isolation and guards ---------------------------------------------------------------

def _isolation():
    """good and bad streams by turns, windows of exact capacity with canaries between them, one
    capacity a byte short, one input past zbytes and one window past out_bytes"""
    good = [e for e in _mixed() if e.fmt != RAW and 0 < len(e.want) <= 65537][::3]
    bad_names = [n for n, _, k in C.CASES if k == "invalid"]
    data = _payload(0, 3000, 5)
    ents = []
    for k, g in enumerate(good):
        ents.append(Ent(g.z, g.fmt, g.want, junk=g.junk))
        name = bad_names[k % len(bad_names)]
        if k % 4 == 1:
            ents.append(Ent(_gz_member(data, crc=7), GZIP, None, E["E_CRC"], cap=3000, mstatus=0, mwant=data))
        elif k % 4 == 3:
            ents.append(Ent(_gz_member(data, isize=5), GZIP, None, E["E_LEN"], cap=3000))
        else:
            ents.append(Ent(C.zstream(name), ZLIB, None, E[C.STATUS[name]], cap=CAP))
    short = _payload(0, 20_000, 6)
    ents.append(Ent(_deflate(short), ZLIB, None, E["E_SZ"], cap=len(short) - 1))
    ents.append(Ent(_deflate(short, wbits=31), GZIP, None, E["E_SZ"], cap=len(short) - 1))
    ents.append(Ent(_deflate(short), ZLIB, short))   # exact capacity passes
    z, desc, out_bytes = _layout(ents)
    # canaries between the windows
    gap = np.arange(len(ents), dtype=np.uint64) * np.uint64(48)
    desc[:, 2] += gap
    out_bytes += int(gap[-1])
    # an input that ends one byte past zbytes, and a window that ends one byte past out_bytes
    past_in = Ent(b"", ZLIB, None, E["E_RANGE"], window=False)
    past_out = Ent(ents[-1].z, ZLIB, None, E["E_RANGE"], mstatus=0, window=False, mwant=short)
    ents += [past_in, past_out]
    extra = np.array([(len(z) - 10, 11, GUARD, 16),
                      (int(desc[-1][0]), int(desc[-1][1]), out_bytes - 100, len(short) + 100)], dtype=np.uint64)
    return ents, (z, np.concatenate([desc, extra]), out_bytes)


def test_isolation_and_guards():
    ents, (z, desc, out_bytes) = _isolation()
    assert sum(e.status == 0 for e in ents) >= 8 and {e.status for e in ents} >= {0, E["E_SZ"], E["E_RANGE"], E["E_CRC"], E["E_LEN"]}
    results, out, rec = _launch(z, desc, D.DMX_BATCH_AUTO, out_bytes)
    _verify(ents, desc, results, out, rec)
    assert rec.nfailed == sum(e.status != 0 for e in ents) and rec.first_bad == 1


# ---- 9. the measure pass ---------------------------------------------------------------------

def _measured(ents):
    """the entries as the measure pass sees them: a wrong gzip CRC passes, with the stored value"""
    out = []
    for e in ents:
        m = Ent(e.z, e.fmt, e.want, e.status, e.junk, e.cap, e.mstatus, e.window)
        if e.mstatus == 0 and e.status != 0:
            m.want = e.mwant
            stored = struct.unpack("<I", e.z[-8:-4])[0] if e.fmt == GZIP else zlib.adler32(m.want)
            m.check = lambda v=stored: v
        out.append(m)
    return out


def test_measure_mixed():
    ents = _mixed()
    for fmt in (D.DMX_BATCH_AUTO, RAW):
        sub = [e for e in ents if (e.fmt == RAW) == (fmt == RAW)]
        z, desc, out_bytes = _layout(sub)
        _run_measure(sub, (z, desc, out_bytes), fmt, f"mixed {fmt}")
        # no limit at all, and a limit one byte short of the longest stream
        desc[:, 3] = NOLIMIT
        _run_measure(sub, (z, desc, out_bytes), fmt, "no limit")
    zl = [e for e in ents if e.fmt == ZLIB]
    z, desc, out_bytes = _layout(zl)
    desc[:, 3] = 200_002
    lim = [Ent(e.z, e.fmt, e.want if len(e.want) <= 200_002 else None, 0 if len(e.want) <= 200_002 else E["E_SZ"], e.junk) for e in zl]
    assert sum(e.status != 0 for e in lim) == 4
    _run_measure(lim, (z, desc, out_bytes), ZLIB, "limit")


@pytest.mark.parametrize("raw", [False, True])
def test_measure_corpus(raw):
    ents = _corpus(raw)
    _run_measure(ents, _layout(ents), RAW if raw else ZLIB, "corpus")


def test_measure_isolation_and_gzip():
    ents, lay = _isolation()
    _run_measure(_measured(ents), lay, D.DMX_BATCH_AUTO, "isolation")
    g = _gzip_cases()
    _run_measure(_measured(g), _layout(g), GZIP, "gzip headers")


# ---- 10. grid shapes -------------------------------------------------------------------------

def _tiny(k):
    data = (b"stream %d " % k) * (1 + k % 5) + bytes([k & 0xFF, k >> 8])
    fmt, wbits = [(ZLIB, 15), (GZIP, 31)][k % 2]
    return Ent(_deflate(data, 1 + k % 9, wbits), fmt, data)


@pytest.mark.parametrize("n", [0, 1, 2, 1100])
def test_grid_shapes(n):
    ents = [_tiny(k) for k in range(n)]
    assert len({e.want for e in ents}) == n
    _run(ents, D.DMX_BATCH_AUTO)


@pytest.mark.parametrize("where", ["first", "last"])
def test_grid_with_one_long_stream(where):
    data = _payload(0, 200_000, 9)
    big = Ent(_deflate(data, 6, 31), GZIP, data)
    ents = [_tiny(k) for k in range(1100)]
    ents = [big] + ents if where == "first" else ents + [big]
    _run(ents, D.DMX_BATCH_AUTO)
    _run_measure(ents, _layout(ents), D.DMX_BATCH_AUTO)


# ---- 11. the Python wrapper --------------------------------------------------------------------

def test_python_wrapper():
    ents = [e for e in _mixed() if e.fmt != RAW][::5]
    datas = [e.want for e in ents]
    out, offsets, results = D.inflate_batch([e.z for e in ents])
    o, off = out.cpu().numpy(), offsets.cpu().tolist()
    assert off == [0] + list(np.cumsum([len(d) for d in datas])) and out.numel() == off[-1]
    for k, d in enumerate(datas):
        assert o[off[k]:off[k + 1]].tobytes() == d
    assert (results["status"] == 0).all() and results["out_len"].tolist() == [len(d) for d in datas]
    assert results["in_used"].tolist() == [len(e.z) - e.junk for e in ents]
    assert results["format"].tolist() == [e.fmt for e in ents] and results["check"].tolist() == [e.check() for e in ents]
    # a tensor with streams, and the lengths given
    z, desc, _ = _layout(ents)
    zt = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    streams = desc[:, :2].astype(np.int64)
    out2, off2, res2 = D.inflate_batch(zt, streams)
    assert torch.equal(out2, out) and torch.equal(off2, offsets) and (res2 == results).all()
    sizes = [len(d) for d in datas]
    out3, off3, res3 = D.inflate_batch(zt, streams, sizes=sizes)
    assert torch.equal(out3, out) and torch.equal(off3, offsets) and (res3 == results).all()
    k = max(range(len(sizes)), key=lambda i: sizes[i])
    sizes[k] -= 1   # too small: -E_SZ for that stream alone
    with pytest.raises(D.DeflateError) as ei:
        D.inflate_batch(zt, streams, sizes=sizes)
    assert ei.value.code == E["E_SZ"] and f"stream {k}" in str(ei.value)
    _, _, res4 = D.inflate_batch(zt, streams, sizes=sizes, strict=False)
    assert res4["status"].tolist() == [E["E_SZ"] if i == k else 0 for i in range(len(sizes))]
    # raw streams by name, and a broken stream among good ones without sizes
    raws = [e for e in _mixed() if e.fmt == RAW][::4]
    out5, off5, res5 = D.inflate_batch([e.z for e in raws], fmt="raw")
    assert out5.cpu().numpy().tobytes() == b"".join(e.want for e in raws) and (res5["format"] == RAW).all()
    parts = [ents[0].z, C.zstream("wrong_adler32"), ents[1].z, ents[2].z[:5]]
    with pytest.raises(D.DeflateError) as ei:
        D.inflate_batch(parts)
    assert ei.value.code == E["E_ZADL32"] and "stream 1" in str(ei.value)
    out6, off6, res6 = D.inflate_batch(parts, strict=False)
    assert res6["status"].tolist() == [0, E["E_ZADL32"], 0, E["E_LEN"]]
    o6, f6 = out6.cpu().numpy(), off6.cpu().tolist()
    assert o6[f6[0]:f6[1]].tobytes() == datas[0] and o6[f6[2]:f6[3]].tobytes() == datas[1]
    with pytest.raises(ValueError):
        D.inflate_batch(parts, fmt="lzma")
    assert D.inflate_batch([])[0].numel() == 0


# ---- 12. graph capture -------------------------------------------------------------------------

def test_batch_in_a_graph():
    """the decode-mode call captured once on a side stream -- kernels only, one after the other -- and
    replayed while the compressed bytes and the descriptors change in place"""
    L = D.lib()
    n, zcap, wcap = 6, 1 << 18, 40_000
    def batch(seed):
        ents = []
        for k in range(n):
            data = _payload((k + seed) % 3, 1000 + 6000 * ((k + seed) % 5) + seed, seed * 10 + k)
            fmt, wbits = [(ZLIB, 15), (GZIP, 31)][(k + seed) % 2]
            ents.append(Ent(_deflate(data, 6, wbits), fmt, data))
        if seed == 3:
            ents[2] = Ent(_gz_member(ents[2].want, crc=5), GZIP, None, E["E_CRC"])
        return ents
    zt = torch.zeros(zcap, dtype=torch.uint8, device="cuda")
    dt = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    res = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.zeros(GUARD + n * wcap + GUARD, dtype=torch.uint8, device="cuda")
    work = torch.empty(int(L.dmx_inflate_batch_work(n)), dtype=torch.uint8, device="cuda")

    def set_input(ents):
        z = b"".join(e.z for e in ents)
        assert len(z) <= zcap
        desc = np.zeros((n, 4), dtype=np.int64)
        off = 0
        for k, e in enumerate(ents):
            desc[k] = (off, len(e.z), GUARD + k * wcap, wcap)
            e.cap = wcap
            off += len(e.z)
        zt[:len(z)].copy_(torch.frombuffer(bytearray(z), dtype=torch.uint8))
        dt.copy_(torch.from_numpy(desc))
        return desc

    def enqueue():
        return D.inflate_batch_async(zt, dt, n, D.DMX_BATCH_AUTO, out, out.numel(), res, work, st)

    first = batch(1)
    set_input(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the kernels are loaded before the capture
        assert enqueue() == 0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r = enqueue()
    assert r == 0
    for seed in (2, 3, 1):
        ents = batch(seed)
        desc = set_input(ents)
        out.fill_(CANARY)
        res.fill_(-1)
        st.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        results = res.cpu().numpy().view(np.uint8).view(D.BRESULT_DTYPE)
        rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
        _verify(ents, desc.astype(np.uint64), results, out.cpu().numpy(), rec, what=f"replay {seed}")
