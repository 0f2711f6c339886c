"""Long runs of equal-size tokens through every kernel that runs the symbol loop's hand-scheduled
path (csrc/dmx_isym.inc): the stream kernel, the batch kernel (decode and measure), the dictionary
batch kernel and the seek-point kernel.  tests/refill_inputs.py builds the streams and
tests/test_refill_inputs.py shows on the CPU that in the "starving" ones every refill of a stretch
of 256 words and more falls between a length and its distance -- the refill that did not rotate
the reader's stream segments (zlib's own streams of megabytes of zeros among them).

Every expected value is zlib's: the data, zlib.adler32, zlib.crc32; the host decoder's status is
the reference of the streams that end early.  The bounded cases come first, in file order: they
give every stream a finite capacity, so a reader that went wrong ends in a status.  The cases
with an unlimited capacity (inflate_batch without sizes=, whose measure pass can only end with the
stream or the input) run behind them, and only when all of those passed."""
import functools
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
import refill_inputs as R

pytestmark = pytest.mark.gpu

E_LEN = -D.E["E_LEN"]
FMT = {"zlib": D.DMX_BATCH_ZLIB, "gzip": D.DMX_BATCH_GZIP, "raw": D.DMX_BATCH_RAW}
CHECK = {"zlib": zlib.adler32, "gzip": zlib.crc32, "raw": lambda d: 0}
WBITS = {"zlib": 15, "gzip": 31, "raw": -15}

_bounded = {}   # bounded case -> passed; the unbounded cases run when every one of them did


def bounded(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        key = (fn.__name__, tuple(a), tuple(sorted(kw.items())))
        _bounded[key] = False
        fn(*a, **kw)
        _bounded[key] = True
    return run


def need_bounded():
    if not _bounded or not all(_bounded.values()):
        pytest.skip("bounded cases did not pass")


# ---- inputs ------------------------------------------------------------------------------------
def by_name(name):
    if "by-name" not in _built:
        _built["by-name"] = {i.name: i for i in R.crafted_inputs() + R.zlib_inputs()}
        assert list(_built["by-name"]) == R.CRAFTED_NAMES + R.ZLIB_NAMES
    return _built["by-name"][name]


def _raw_of(i):
    assert i.fmt == "zlib"
    return i.z[2:-4]


_built = {}
BATCH_KEYS = ["crafted", "zlib", "raw"]


def batch(key):
    """(fmt of the call, [(stream, its format, data)]) of one of BATCH_KEYS: a text stream on each side of
    every other stream.  "raw": zlib's 1 MiB of zeros as a raw stream and the bodies of three
    crafted streams (at an aligned address their bit offsets move by 16, a multiple of every T)."""
    if "batches" in _built:
        return _built["batches"][key]
    tz, t = R.text_stream()
    traw = zlib.compress(t, 6)[2:-4]
    out = {}
    BY_NAME = {n: by_name(n) for n in R.CRAFTED_NAMES + R.ZLIB_NAMES}
    for k, fmt, items in (
            ("crafted", "zlib", [(i.z, "zlib", i.data) for i in R.crafted_inputs()]),
            ("zlib", "auto", [(i.z, i.fmt, i.data) for i in R.zlib_inputs() if i.fmt != "raw"]),
            ("raw", "raw", [(BY_NAME["zeros-1m-raw"].z, "raw", BY_NAME["zeros-1m-raw"].data)] +
             [(_raw_of(BY_NAME[n]), "raw", BY_NAME[n].data) for n in ("t2-zero-starving", "t16-starving", "t4-at-end")])):
        text = (traw, "raw", t) if fmt == "raw" else (tz, "zlib", t)
        ents = [text]
        for it in items:
            ents += [it, text]
        out[k] = (fmt, ents)
    assert list(out) == BATCH_KEYS
    _built["batches"] = out
    return out[key]


def pack(streams):
    """(CUDA tensor, (n, 2) int64 of (off, len)): every stream at a 4-byte aligned offset -- the
    alignment the CPU model qualifies the 16-bit geometries at -- with junk in the gaps"""
    buf, offs = bytearray(), []
    for z in streams:
        buf += b"\xee" * (-len(buf) % 4)
        offs.append((len(buf), len(z)))
        buf += z
    zt = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    assert zt.data_ptr() % 4 == 0
    return zt, np.array(offs, dtype=np.int64)


def check_batch(ents, out, offsets, results, what):
    off = offsets.cpu().numpy()
    got = out.cpu().numpy()
    for k, (z, fmt, data) in enumerate(ents):
        r = results[k]
        rec = (int(r["status"]), int(r["format"]), int(r["out_len"]), int(r["in_used"]), int(r["check"]))
        assert rec == (0, FMT[fmt], len(data), len(z), CHECK[fmt](data)), (what, k, rec)
        assert off[k + 1] - off[k] == len(data), (what, k)
        assert got[off[k]:off[k + 1]].tobytes() == data, (what, k, "bytes differ")


# ---- bounded -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CRAFTED_NAMES + [n for n in R.ZLIB_NAMES if not n.endswith(("-gzip", "-raw"))])
@bounded
def test_stream_kernel(name):
    i = by_name(name)
    zt = torch.frombuffer(bytearray(i.z), dtype=torch.uint8).cuda()
    out, status = D.inflate_gpu(zt, len(i.data) + 16)
    assert status == 0, (name, status)
    assert out.numel() == len(i.data) and out.cpu().numpy().tobytes() == i.data, name


@pytest.mark.parametrize("key", BATCH_KEYS)
@bounded
def test_batch_with_sizes(key):
    fmt, ents = batch(key)
    zt, offs = pack([e[0] for e in ents])
    out, offsets, results = D.inflate_batch(zt, streams=offs, fmt=fmt, sizes=[len(e[2]) for e in ents], strict=False)
    check_batch(ents, out, offsets, results, key)


@pytest.mark.parametrize("key", BATCH_KEYS)
@bounded
def test_batch_measure_exact_capacity(key):
    """dmx_inflate_batch_async under DMX_BATCH_MEASURE, out NULL, out_cap the exact length"""
    fmt, ents = batch(key)
    zt, offs = pack([e[0] for e in ents])
    n = len(ents)
    desc = np.zeros((n, 4), dtype=np.int64)
    desc[:, :2] = offs
    desc[:, 3] = [len(e[2]) for e in ents]
    dt = torch.from_numpy(desc).cuda()
    res = torch.full((n * 4,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(int(D.lib().dmx_inflate_batch_work(n)), dtype=torch.uint8, device="cuda")
    flags = {"auto": D.DMX_BATCH_AUTO, **FMT}[fmt] | D.DMX_BATCH_MEASURE
    assert D.inflate_batch_async(zt, dt, n, flags, None, 0, res, work, st) == 0
    torch.cuda.synchronize()
    results = res.cpu().numpy().view(np.uint8).view(D.BRESULT_DTYPE)[:n]
    for k, (z, f, data) in enumerate(ents):
        r = results[k]
        rec = (int(r["status"]), int(r["format"]), int(r["out_len"]), int(r["in_used"]), int(r["check"]))
        assert rec == (0, FMT[f], len(data), len(z), CHECK[f](data)), (key, k, rec)
    rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    assert (rec.nfailed, rec.total_out) == (0, sum(len(e[2]) for e in ents)), key


def _dict_batch():
    zdict, streams = R.dict_inputs()
    _, t = R.text_stream()
    c = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=zdict)
    traw = c.compress(t) + c.flush()
    ents = [(traw, "raw", t)]
    for _, raw, data in streams:
        ents += [(raw, "raw", data), (traw, "raw", t)]
    return zdict, ents


@bounded
def test_dictionary_batch_with_sizes():
    """raw streams whose first matches read the preset dictionary's last bytes"""
    zdict, ents = _dict_batch()
    zt, offs = pack([e[0] for e in ents])
    out, offsets, results = D.inflate_batch(zt, streams=offs, fmt="raw", zdict=zdict, sizes=[len(e[2]) for e in ents],
                                            strict=False)
    check_batch(ents, out, offsets, results, "dict")


@pytest.mark.parametrize("name", ["zeros-768k", "zeros-1m", "zeros-5m", "A-5m", "zeros-16m"])
@bounded
def test_seek_points_zlib_streams(name):
    """a point per 1 MiB of output at the next block boundary: zlib's blocks of constant input hold
    about 4.2 MB, so the 16 MiB stream has 3 points and more, the first with the starving block"""
    i = by_name(name)
    ix = D.zindex_build(i.z, span=1 << 20)
    n = len(i.data)
    if name == "zeros-16m":
        assert ix.npoints >= 3 and int(ix.points["out_len"][0]) > 4_000_000
    assert ix.out_len == n
    zt = torch.frombuffer(bytearray(i.z), dtype=torch.uint8).cuda()
    out = D.inflate_indexed(zt, ix, verify=True)
    assert out.numel() == n and out.cpu().numpy().tobytes() == i.data, name
    first = int(ix.points["out_len"][0])
    ranges = [(100, 1000), (first // 2, 70_000), (max(0, first - 30_000), min(60_000, n - max(0, first - 30_000))),
              (n - 1000, 1000), (0, min(n, first + 1))]
    for off, ln in ranges:   # inside the starving block, across its end, at the stream's end
        got = D.zindex_pread(zt, ix, off, ln, verify=True)
        assert got.cpu().numpy().tobytes() == i.data[off:off + ln], (name, off, ln)


@bounded
def test_seek_points_crafted_streams():
    """a point behind every block that produced output (span 1)"""
    for i in R.crafted_inputs():
        ix = D.zindex_build(i.z, span=1)
        zt = torch.frombuffer(bytearray(i.z), dtype=torch.uint8).cuda()
        out = D.inflate_indexed(zt, ix, verify=True)
        assert out.cpu().numpy().tobytes() == i.data, i.name
        mid = len(i.data) // 2
        got = D.zindex_pread(zt, ix, mid - 500, 1000, verify=True)
        assert got.cpu().numpy().tobytes() == i.data[mid - 500:mid + 500], i.name


# ---- unbounded: behind the bounded cases, and only when they all passed -------------------------
@pytest.mark.parametrize("key", BATCH_KEYS)
def test_batch_without_sizes(key):
    """the measure pass with out_cap = UINT64_MAX, then the decode: what the sized call gives"""
    need_bounded()
    fmt, ents = batch(key)
    zt, offs = pack([e[0] for e in ents])
    out, offsets, results = D.inflate_batch(zt, streams=offs, fmt=fmt, strict=False)
    check_batch(ents, out, offsets, results, key)
    out2, offsets2, results2 = D.inflate_batch(zt, streams=offs, fmt=fmt, sizes=[len(e[2]) for e in ents], strict=False)
    assert torch.equal(out, out2) and torch.equal(offsets, offsets2), key
    assert results.tobytes() == results2.tobytes(), key


def test_dictionary_batch_without_sizes():
    need_bounded()
    zdict, ents = _dict_batch()
    zt, offs = pack([e[0] for e in ents])
    out, offsets, results = D.inflate_batch(zt, streams=offs, fmt="raw", zdict=zdict, strict=False)
    check_batch(ents, out, offsets, results, "dict")


def _host_status(z):
    try:
        D.deflate_decompress(z)
    except D.DeflateError as e:
        return e.code
    return 0


@pytest.mark.parametrize("with_dict", [False, True])
def test_cut_streams_end_with_the_input(with_dict):
    """streams cut inside a dynamic block whose all-zero code is a literal, a length (with an
    all-zero distance code) or the end of block, and the text stream cut at 10 places inside block
    bodies: the reader's zeros behind the cut spell tokens, and without a capacity only the end of
    the input stops the measure pass.  -E_LEN each, as on the host; the neighbours decode."""
    need_bounded()
    cuts = R.cut_inputs()
    tz, t = R.text_stream()
    streams, want = [tz], [None]
    for name, z in cuts:
        streams += [z, tz]
        want += [name, None]
    kw = {"zdict": R.dict_inputs()[0]} if with_dict else {}
    out, offsets, results = D.inflate_batch(streams, strict=False, **kw)
    off = offsets.cpu().numpy()
    got = out.cpu().numpy()
    for k, name in enumerate(want):
        r = results[k]
        if name is None:
            rec = (int(r["status"]), int(r["out_len"]), int(r["in_used"]), int(r["check"]))
            assert rec == (0, len(t), len(tz), zlib.adler32(t)), (k, rec)
            assert got[off[k]:off[k + 1]].tobytes() == t, k
        else:
            host = _host_status(streams[k])
            assert host == E_LEN, (name, host)
            assert int(r["status"]) == E_LEN, (name, int(r["status"]))
            assert (int(r["out_len"]), int(r["in_used"]), int(r["check"])) == (0, 0, 0), (name, r)
