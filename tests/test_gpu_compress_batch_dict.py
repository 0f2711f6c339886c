"""Batches of independent buffers against preset dictionaries on the GPU
(dmx_encode_batch_dict_async, compress_batch(zdict=)).  The specification: the bytes of stream k are
what the single encode writes for buffer k alone with the same options and its dictionary, so every
stream is compared byte for byte with D.compress(buf, dict=True, pre=d, ...) and with the CPU
oracle's compress(dict=True, pre=d) under the stream's header, and is round-tripped through zlib
(zdict=d) and through inflate_batch(zdict=, dict_of=).  sw = 1024 so that block edges cost
kilobytes; sw = 32768 where the size itself matters."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
from oracle import oracle as O

pytestmark = pytest.mark.gpu

E = D.E
SENT = 0xA5
NODICT = D.DMX_BATCH_NODICT
Z, RAW, DICT, FD = D.DMX_ZLIB, D.DMX_F_FINAL, D.DMX_F_DICT, D.DMX_F_FDICT
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the project's generator with two seeds: the buffers from one, the dictionaries from the other
_TEXT = D.gen_text(1 << 18, 21).tobytes()
_PRE = D.gen_text(1 << 17, 22).tobytes()
_RAND = D.gen_random(1 << 16, 11).tobytes()


def _buf(n, salt):
    o = (salt * 7919) % 100000
    return _TEXT[o:o + n]


def _pre(n, salt=0):
    o = (salt * 4099) % 60000
    return _PRE[o:o + n]


@pytest.fixture(scope="module")
def enc():
    e = D.Encoder(0, 1 << 20)
    yield e
    e.close()


def _lay(bufs, first=0):
    """the parts in one tensor, part k at an offset that is (first + k) mod 16, junk between them"""
    parts, desc, cur = [], [], 0
    for k, b in enumerate(bufs):
        gap = (first + k - cur) % 16
        parts.append(bytes([0xEE]) * gap)
        cur += gap
        desc.append((cur, len(b)))
        parts.append(b)
        cur += len(b)
    parts.append(bytes([0xEE]) * 17)
    t = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, np.array(desc, dtype=np.int64).reshape(-1, 2)


def _di(v):
    """a dict_of entry as a list index, None for none"""
    return None if v is None or v < 0 or v == NODICT else int(v)


def _of_array(dict_of):
    return np.array([NODICT if _di(v) is None else _di(v) for v in dict_of], dtype=np.uint32)


def _batch(enc, t, desc, dict_t, ddesc, dict_of, opts, max_blocks=None, out_cap=None, expect_rc=0):
    """one dmx_encode_batch_dict_async call on a sentinel-filled output; returns (out bytes, results, record)"""
    L = D.lib()
    n, nd = desc.shape[0], ddesc.shape[0]
    sw = opts.sw or 32768
    if max_blocks is None:
        max_blocks = D.encode_batch_blocks(desc[:, 1].tolist(), sw)
    cap = int(L.dmx_encode_batch_dict_bound(int(desc[:, 1].clip(0, t.numel()).sum()), n, sw, opts.flags))
    out = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    if out_cap is None:
        out_cap = cap
    enc.reserve_batch_dict(max_blocks, n, nd, sw, opts.flags)
    dt = torch.from_numpy(np.ascontiguousarray(desc)).cuda() if n else torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    ddt = torch.from_numpy(np.ascontiguousarray(ddesc)).cuda() if nd else None
    oft = torch.from_numpy(_of_array(dict_of).view(np.int32).copy()).cuda() if dict_of is not None else None
    res = torch.full((max(n, 1) * 4,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()   # (on the default stream the call runs on the encoder's own stream)
    rc = D.compress_batch_dict_async(enc, t, dt, n, max_blocks, dict_t, ddt, nd, oft, out, out_cap, res, st, opts)
    assert rc == expect_rc, rc
    torch.cuda.synchronize()
    results = res.cpu().numpy()[:4 * n].view(np.uint8).reshape(-1).view(D.ERESULT_DTYPE)
    rec = D.EBatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    return out.cpu().numpy(), results, rec


_single_cache = {}


def _single(buf, d, opts):
    """the specification: the single encode of buf alone with the same opts and its dictionary d (None:
    none, written as with DMX_F_FDICT cleared)"""
    key = (buf, d, opts.sw, opts.max_chain, opts.flags)
    if key not in _single_cache:
        fl = opts.flags if d is not None else opts.flags & ~FD
        _single_cache[key] = D.compress(buf, sw=opts.sw, max_chain=opts.max_chain, flags=fl, pre=d if d else None, dict=True)
    return _single_cache[key]


def _oracle(buf, d, opts):
    """the oracle's stream with the header exchanged: 78 BB + DICTID where the stream names a dictionary"""
    fl, sw = opts.flags, opts.sw
    z = O.compress(buf, sw=sw, max_chain=opts.max_chain, lazy=bool(fl & D.DMX_F_LAZY), dict=True,
                   pre=d[-sw:] if d else None, store_check=bool(fl & D.DMX_F_STORE_CHECK), flags=fl & 7,
                   deep=bool(fl & D.DMX_F_DEEP))
    if (fl & FD) and d is not None:
        assert z[:2] == b"\x78\x9c"
        z = b"\x78\xbb" + struct.pack(">I", zlib.adler32(d)) + z[2:]
    return z


def _inflate_host(z, d, opts, n):
    """zlib's reading of the stream with the dictionary d"""
    fl = opts.flags
    if (fl & FD) and d is not None:
        o = zlib.decompressobj(zdict=d)
        out = o.decompress(z)
        assert o.eof and not o.unused_data
        return out
    body = z[2:-4] if fl & D.DMX_F_HEADER else z   # (78 9C over a history: only the body is zlib's to read)
    o = zlib.decompressobj(-15, zdict=d[-32768:]) if d else zlib.decompressobj(-15)
    out = o.decompress(body) + o.flush()
    assert o.eof and not o.unused_data
    if fl & D.DMX_F_HEADER:
        assert z[:2] == b"\x78\x9c" and z[-4:] == struct.pack(">I", zlib.adler32(out))
    return out


def _verify(bufs, dicts, dict_of, opts, outb, results, rec, what="", oracle=True, device_trip=True):
    """every stream against the single encode, the oracle and zlib; the batch through inflate_batch"""
    pos, zs = 0, []
    for k, data in enumerate(bufs):
        di = (0 if dicts else None) if dict_of is None else _di(dict_of[k])
        d = None if di is None else dicts[di]
        r = results[k]
        assert r["status"] == 0, (what, k, r)
        assert int(r["out_off"]) == pos, (what, k, int(r["out_off"]), pos)
        got = outb[pos:pos + int(r["out_len"])].tobytes()
        want = _single(data, d, opts)
        assert got == want, (what, k, len(data), len(got), len(want))
        if oracle:
            assert got == _oracle(data, d, opts), (what, k, "oracle")
        assert _inflate_host(got, d, opts, len(data)) == data, (what, k)
        if opts.flags & D.DMX_F_HEADER:
            assert got[:2] == (b"\x78\xbb" if (opts.flags & FD) and d is not None else b"\x78\x9c"), (what, k)
            if (opts.flags & FD) and d is not None:
                assert got[2:6] == struct.pack(">I", zlib.adler32(d)), (what, k, "DICTID")
        assert int(r["check"]) == (zlib.adler32(data) if opts.flags & D.DMX_F_TRAILER else 0), (what, k)
        zs.append(got)
        pos += int(r["out_len"])
    assert rec.status == 0 and rec.nfailed == 0 and rec.first_bad == 0xFFFFFFFF, (what, rec.status, rec.nfailed)
    assert rec.out_len == pos and rec.in_len == sum(len(b) for b in bufs), (what, rec.out_len, pos)
    assert (outb[(pos + 3) & ~3:] == SENT).all(), (what, "a byte at or beyond align4(out_len) was written")
    # the project's own batch decoder, where the streams tell it what it needs (FDICT, or raw)
    if device_trip and dicts and ((opts.flags & FD) or not (opts.flags & D.DMX_F_HEADER)):
        of = [0] * len(bufs) if dict_of is None else [-1 if _di(v) is None else _di(v) for v in dict_of]
        back, boffs, bres = D.inflate_batch(zs, fmt="zlib" if opts.flags & D.DMX_F_HEADER else "raw", zdict=list(dicts), dict_of=of)
        bo, flat = boffs.cpu().numpy(), back.cpu().numpy().tobytes()
        for k, b in enumerate(bufs):
            assert flat[bo[k]:bo[k] + int(bres[k]["out_len"])] == b, (what, k, "inflate_batch")


def _run_and_verify(enc, bufs, dicts, dict_of, opts, what="", first=0, dfirst=0, **kw):
    t, desc = _lay(bufs, first)
    dict_t, ddesc = _lay(dicts, dfirst) if dicts else (None, np.zeros((0, 2), dtype=np.int64))
    outb, results, rec = _batch(enc, t, desc, dict_t, ddesc, dict_of, opts)
    _verify(bufs, dicts, dict_of, opts, outb, results, rec, what, **kw)
    return outb, results, rec


FRAMINGS = {"zlib_fdict": Z | DICT | FD, "zlib": Z | DICT, "raw": RAW | DICT}
LENS_1K = [0, 1, 2, 3, 1023, 1024, 1025, 2048, 3 * 1024 + 5]


@pytest.mark.parametrize("framing", sorted(FRAMINGS))
def test_lengths(enc, framing):
    """0, 1, 2, 3, sw - 1, sw, sw + 1, 2 sw, 3 sw + 5 in one batch against one dictionary"""
    bufs = [_buf(n, 3 + j) for j, n in enumerate(LENS_1K)]
    opts = D.Opts(1024, 7, FRAMINGS[framing] | D.DMX_F_LAZY, 0)
    outb, results, rec = _run_and_verify(enc, bufs, [_pre(300)], None, opts, framing)
    assert rec.nblocks == D.encode_batch_blocks(LENS_1K, 1024) == sum(int(x["nblocks"]) for x in results)
    r = enc.result()   # dmx_encode_result after a batch: the totals
    assert (r.out_len, r.n, r.adler, r.status) == (rec.out_len, rec.in_len, 0, 0)
    idx = torch.zeros(3 * 64, dtype=torch.int64, device="cuda")
    assert D.lib().dmx_block_index(enc._ctx, idx.data_ptr(), 64, None) == -E["E_INVAL"]


@pytest.mark.parametrize("fdict", [True, False])
def test_dictionary_lengths_and_alignments(enc, fdict):
    """dictionaries of 1, 2, 3, 300, sw (and sw + 1 without FDICT: its last sw bytes) at every offset
    residue mod 16 in d_dict; the streams' offsets take every residue too"""
    lens = [1, 2, 3, 300, 1024] + ([] if fdict else [1025])
    dicts = [_pre(lens[j % len(lens)], j) for j in range(16 + len(lens))]
    bufs = [_buf((700, 1024, 1500, 2100)[k % 4], k) for k in range(len(dicts))]
    t, desc = _lay(bufs, 5)
    dict_t, ddesc = _lay(dicts, 3)
    assert {int(o) % 16 for o in ddesc[:, 0]} == set(range(16)) == {int(o) % 16 for o in desc[:, 0]}
    opts = D.Opts(1024, 7, Z | DICT | (FD if fdict else 0) | D.DMX_F_LAZY, 0)
    of = list(range(len(dicts)))
    outb, results, rec = _batch(enc, t, desc, dict_t, ddesc, of, opts)
    _verify(bufs, dicts, of, opts, outb, results, rec, f"fdict={fdict}")


def test_full_window_dictionary(enc):
    """sw = 32768 against a dictionary of 32 768 bytes: one block and multi-block streams"""
    d = _pre(32768, 1)
    bufs = [_buf(4096, 1), _buf(40000, 2), _buf(32768, 3)]
    for fl in (Z | DICT | FD, RAW | DICT):
        _run_and_verify(enc, bufs, [d], None, D.Opts(32768, 7, fl | D.DMX_F_LAZY, 0), hex(fl), first=7, dfirst=9)


def test_wrong_predecessor(enc):
    """the same 3 KiB buffer twice without a dictionary: stream 1's first block must not search stream
    0's last block, which precedes it in the table and holds the same bytes"""
    b = _buf(3072, 9)
    for fl in (Z | DICT | FD, Z | DICT, RAW | DICT):
        opts = D.Opts(1024, 7, fl | D.DMX_F_LAZY, 0)
        outb, results, rec = _run_and_verify(enc, [b, b], [_pre(300)], [NODICT, NODICT], opts, hex(fl))
        z1 = outb[int(results[1]["out_off"]):][:int(results[1]["out_len"])].tobytes()
        assert z1 == D.compress(b, sw=1024, max_chain=7, flags=fl & ~FD, lazy=True, dict=True)
        assert (zlib.decompress(z1) if fl & D.DMX_F_HEADER else zlib.decompress(z1, -15)) == b
        assert z1 == outb[:int(results[0]["out_len"])].tobytes()


def test_several_dictionaries(enc):
    dicts = [_pre(300, 1), _pre(1024, 2), _pre(77, 3)]
    of = [0, 0, 1, -1, 1, 2, 0]
    bufs = [_buf(n, 11 + k) for k, n in enumerate([600, 2500, 1024, 3000, 5, 2049, 0])]
    for name, fl in sorted(FRAMINGS.items()):
        opts = D.Opts(1024, 7, fl | D.DMX_F_LAZY, 0)
        outb, results, rec = _run_and_verify(enc, bufs, dicts, of, opts, name, first=2, dfirst=11)
        if fl & FD:
            heads = [outb[int(r["out_off"]):][:6].tobytes() for r in results]
            assert heads[3][:2] == b"\x78\x9c"
            for k in (0, 1, 2, 4, 5, 6):
                assert heads[k] == b"\x78\xbb" + struct.pack(">I", zlib.adler32(dicts[of[k]])), k
        # d_dict_of NULL: every stream uses dictionary 0; with no dictionary at all, none
        _run_and_verify(enc, bufs, dicts[:1], None, opts, name + " NULL of")
        _run_and_verify(enc, bufs, [], None, opts, name + " ndicts 0")


OPTSETS = {
    "exhaustive": (0, 0),
    "k3": (3, 0), "k6": (6, 0), "k7": (7, 0), "k8": (8, 0), "k12": (12, 0),
    "k7_lazy": (7, D.DMX_F_LAZY),
    "k7_lazy_deep_store_check": (7, D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK),
    "exact_sort": (7, D.DMX_F_EXACT_SORT),
}


@pytest.mark.parametrize("optset", sorted(OPTSETS))
def test_option_sets(enc, optset):
    """every history-group instantiation (6, 7, 8 candidates; K > 8 in groups), the exhaustive walk,
    lazy, deep, the store check and the exact sort, under FDICT and raw framing"""
    k, extra = OPTSETS[optset]
    dicts = [_pre(1024, 4), _pre(300, 5)]
    of = [0, 1, -1, 0, 1]
    bufs = [_buf(n, 21 + j) for j, n in enumerate([1500, 1024, 2048, 700, 3077])]
    for fl in (Z | DICT | FD, RAW | DICT):
        _run_and_verify(enc, bufs, dicts, of, D.Opts(1024, k, fl | extra, 0), f"{optset}/{fl:x}")


def test_noise_first_block_under_store_check(enc):
    """a noise buffer as a first block (stored by K0, which a dictionary does not change), then text"""
    opts = D.Opts(8192, 7, Z | DICT | FD | D.DMX_F_LAZY | D.DMX_F_STORE_CHECK, 0)
    bufs = [_RAND[:8192] + _buf(5000, 1), _buf(8192, 2), _RAND[100:8292], bytes(8192) + _buf(100, 3)]
    _run_and_verify(enc, bufs, [_pre(8192, 6)], None, opts)
    assert enc.result().nstored >= 2


def _loop_case(period):
    bufs = [_buf(600, k % 250) for k in range(2000)]
    dicts = [_pre(1024, 7), _pre(900, 8)]
    of = [(k // period) % 2 for k in range(2000)]
    return bufs, dicts, of


@pytest.mark.parametrize("period", [1, 2, 97])
def test_loop_edges_resident_and_simple(enc, period):
    """more table entries than workgroups of the history loop: 2 000 streams of 600 B at sw 1024 with
    the dictionary changing every `period` streams; the resident form and the simple form (a workgroup
    per entry, through the hook) give the same bytes"""
    bufs, dicts, of = _loop_case(period)
    grid = (ctypes.c_uint32 * 1)(0)
    D.lib().dmx_encode_batch_dict_geometry(grid)
    assert 0 < grid[0] < len(bufs)
    t, desc = _lay(bufs)
    dict_t, ddesc = _lay(dicts, 13)
    opts = D.Opts(1024, 7, Z | DICT | FD | D.DMX_F_LAZY, 0)
    runs = []
    try:
        for simple in (0, 1):
            enc.set_hook("bdict_simple", simple)
            outb, results, rec = _batch(enc, t, desc, dict_t, ddesc, of, opts)
            runs.append((outb.tobytes(), results.tobytes(), bytes(rec)))
    finally:
        enc.set_hook("bdict_simple", 0)
    assert runs[0] == runs[1]
    outb, results, rec = _batch(enc, t, desc, dict_t, ddesc, of, opts)
    _verify(bufs, dicts, of, opts, outb, results, rec, f"period {period}")


def test_void_entries_capacities_and_bad_streams(enc):
    dicts = [_pre(300, 1), _pre(1024, 2)]
    bufs = [_buf(n, 40 + k) for k, n in enumerate([600, 2500, 1024, 0, 3000, 77])]
    of = [0, 1, -1, 0, 1, 0]
    t, desc = _lay(bufs, 1)
    # the dictionaries' records: two good ones, then one past the end, one whose off + len wraps, an
    # empty one and one of sw + 1 bytes
    dict_t, ddesc = _lay(dicts + [_pre(1025, 3)], 4)
    ddesc = np.concatenate((ddesc[:2], [[dict_t.numel() - 2, 3], [-8, 16], [5, 0]], ddesc[2:]))
    opts = D.Opts(1024, 7, Z | DICT | FD | D.DMX_F_LAZY, 0)
    exact = D.encode_batch_blocks([len(b) for b in bufs], 1024)
    good, gres, grec = _batch(enc, t, desc, dict_t, ddesc, of, opts)
    _verify(bufs, dicts, of, opts, good, gres, grec, "good")
    # void entries: max_blocks above the need
    for mb in (exact + 1, 2 * exact + 7):
        outb, results, rec = _batch(enc, t, desc, dict_t, ddesc, of, opts, max_blocks=mb)
        assert (outb.tobytes(), results.tobytes(), bytes(rec)) == (good.tobytes(), gres.tobytes(), bytes(grec))
    # -E_SZ for max_blocks: the record holds the need, no byte written
    outb, results, rec = _batch(enc, t, desc, dict_t, ddesc, of, opts, max_blocks=exact - 1)
    assert rec.status == -E["E_SZ"] and rec.nblocks == exact and (outb == SENT).all()
    # ... and for out_cap
    a4 = (grec.out_len + 3) & ~3
    outb, results, rec = _batch(enc, t, desc, dict_t, ddesc, of, opts, out_cap=a4)
    assert rec.status == 0 and outb[:rec.out_len].tobytes() == good[:rec.out_len].tobytes() and (outb[a4:] == SENT).all()
    outb, results, rec = _batch(enc, t, desc, dict_t, ddesc, of, opts, out_cap=a4 - 4)
    assert rec.status == -E["E_SZ"] and rec.out_len == grec.out_len and rec.nblocks == exact and (outb == SENT).all()
    assert (results["out_off"] == gres["out_off"]).all() and (results["out_len"] == gres["out_len"]).all()
    # bad streams of every kind among the good ones: a buffer outside d_in, an index >= ndicts, a record
    # past the end, a record that wraps, and under FDICT a dictionary of length 0 and one of sw + 1
    ins = [1, 1, 3, 4, 6, 6]
    bad_desc = np.insert(desc, ins, [[t.numel() - 2, 3], [0, 100], [0, 100], [16, 50], [32, 10], [48, 1100]], axis=0)
    bad_of = list(np.insert(np.array(of, dtype=np.int64), ins, [0, 6, 2, 3, 4, 5]))
    want = [-E["E_RANGE"]] * 4 + [-E["E_INVAL"]] * 2
    where = [1, 2, 5, 7, 10, 11]
    outb, results, rec = _batch(enc, t, bad_desc, dict_t, ddesc, bad_of, opts, max_blocks=exact)
    assert rec.status == 0 and rec.nfailed == 6 and rec.first_bad == 1
    assert rec.out_len == grec.out_len and rec.in_len == grec.in_len and rec.nblocks == grec.nblocks
    assert outb[:rec.out_len].tobytes() == good[:grec.out_len].tobytes()
    for k, w in zip(where, want):
        assert (results[k]["status"], results[k]["out_len"], results[k]["nblocks"]) == (w, 0, 0), k
    assert np.delete(results, where).tobytes() == gres.tobytes()
    offs = np.concatenate((results["out_off"], [rec.out_len])).astype(np.int64)
    assert (np.diff(offs) == results["out_len"].astype(np.int64)).all()
    # without FDICT the last two are good streams: no history, and the last sw bytes
    o2 = D.Opts(1024, 7, RAW | DICT | D.DMX_F_LAZY, 0)
    outb, results, rec = _batch(enc, t, bad_desc, dict_t, ddesc, bad_of, o2, max_blocks=exact + 3)
    assert rec.nfailed == 4 and results[10]["status"] == 0 and results[11]["status"] == 0
    tb = t.cpu().numpy().tobytes()
    z10 = outb[int(results[10]["out_off"]):][:int(results[10]["out_len"])].tobytes()
    z11 = outb[int(results[11]["out_off"]):][:int(results[11]["out_len"])].tobytes()
    assert z10 == _single(tb[32:42], None, o2)
    assert z11 == _single(tb[48:1148], _pre(1025, 3), o2) == _oracle(tb[48:1148], _pre(1025, 3), o2)


SCAN_TILE = 256   # table entries per workgroup of K3 (csrc: SCAN_TILE)


def test_scan3_hook_across_tiles(enc):
    """K3's two launch shapes (one launch per tile that composes the aggregates itself; the scan3 hook's
    scan by one workgroup + apply) give the same bytes on a dictionary batch whose 525 blocks span
    three scan tiles: 300 buffers of 0 to 2 500 bytes at sw 1024 that name dictionary 0, dictionary 1
    or none in turn (48-bit and 16-bit headers in one scan), one of them empty, one refused; stream 148
    begins a tile and stream 147 ends the tile before it.  With max_blocks exact and with a whole void
    tile behind the real blocks, and under -E_SZ for out_cap."""
    n, bad, empty = 300, 101, 60
    lens = [(k * 977 + 311) % 2501 for k in range(n)]
    lens[empty] = 0
    bufs = [_buf(m, 100 + k) for k, m in enumerate(lens)]
    dicts = [_pre(1024, 12), _pre(300, 13)]
    of = [(0, 1, NODICT)[k % 3] for k in range(n)]
    t, desc = _lay(bufs, 6)
    dict_t, ddesc = _lay(dicts, 9)
    desc[bad] = [t.numel() + 5, 10]   # in_off beyond the input
    # the plan, which is deterministic: a refused stream has no blocks, every other max(1, ceil(len / sw))
    nb = [0 if k == bad else max(1, -(-m // 1024)) for k, m in enumerate(lens)]
    starts = np.concatenate(([0], np.cumsum(nb)))
    exact = int(starts[-1])
    assert exact > 2 * SCAN_TILE and min(lens) == 0 and max(lens) <= 2500
    firsts = [k for k in range(1, n) if nb[k] and starts[k] % SCAN_TILE == 0]
    lasts = [k for k in range(n) if nb[k] and starts[k + 1] % SCAN_TILE == 0]
    assert firsts == [148] and lasts == [147] and of[148] == 1 and of[147] == 0 and of[empty] == 0
    assert {of[k] for k in range(n) if k != bad} == {0, 1, NODICT}
    opts = D.Opts(1024, 7, Z | DICT | FD | D.DMX_F_LAZY, 0)
    runs, short = {}, {}
    try:
        for scan3 in (0, 1):
            enc.set_hook("scan3", scan3)
            for mb in (exact, exact + SCAN_TILE):
                outb, results, rec = _batch(enc, t, desc, dict_t, ddesc, of, opts, max_blocks=mb)
                runs[scan3, mb] = (outb.tobytes(), results.tobytes(), bytes(rec))
                assert rec.status == 0 and rec.nblocks == exact and rec.nfailed == 1 and rec.first_bad == bad
                a4 = (rec.out_len + 3) & ~3
                sb, sres, srec = _batch(enc, t, desc, dict_t, ddesc, of, opts, max_blocks=mb, out_cap=a4 - 4)
                assert srec.status == -E["E_SZ"] and srec.out_len == rec.out_len and (sb == SENT).all(), (scan3, mb)
                short[scan3, mb] = (sres.tobytes(), bytes(srec))
    finally:
        enc.set_hook("scan3", 0)
    assert len(set(runs.values())) == 1 and len(set(short.values())) == 1
    outb, results, rec = _batch(enc, t, desc, dict_t, ddesc, of, opts, max_blocks=exact)
    assert (outb.tobytes(), results.tobytes(), bytes(rec)) == runs[0, exact]
    pos = 0
    for k, data in enumerate(bufs):
        r = results[k]
        assert int(r["out_off"]) == pos, k
        if k == bad:
            assert (r["status"], r["out_len"], r["nblocks"]) == (-E["E_RANGE"], 0, 0)
            continue
        assert r["status"] == 0 and r["nblocks"] == nb[k], k
        got = outb[pos:pos + int(r["out_len"])].tobytes()
        assert got == _single(data, None if of[k] == NODICT else dicts[of[k]], opts), (k, len(data))
        pos += int(r["out_len"])
    assert rec.out_len == pos and (outb[(pos + 3) & ~3:] == SENT).all()


def test_graph_replays_with_rewritten_dictionary(enc):
    """one call captured and replayed twice with the dictionary bytes rewritten between the replays:
    the second output names (DICTID) and uses the new dictionary"""
    bufs = [_buf(n, 60 + k) for k, n in enumerate([3000, 0, 1024, 700])]
    d0, d1 = _pre(500, 10), _pre(500, 11)
    t, desc = _lay(bufs, 3)
    dict_t, ddesc = _lay([d0], 5)
    opts = D.Opts(1024, 7, Z | DICT | FD | D.DMX_F_LAZY, 0)
    n, mb = len(bufs), D.encode_batch_blocks([len(b) for b in bufs], 1024)
    cap = int(D.lib().dmx_encode_batch_dict_bound(sum(len(b) for b in bufs), n, 1024, opts.flags))
    enc.reserve_batch_dict(mb, n, 1, 1024, opts.flags)
    dt, ddt = torch.from_numpy(desc).cuda(), torch.from_numpy(ddesc).cuda()
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    res = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")

    def enqueue():
        return D.compress_batch_dict_async(enc, t, dt, n, mb, dict_t, ddt, 1, None, out, cap, res, st, opts)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the kernels are loaded before the capture
        assert enqueue() == 0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r = enqueue()
    assert r == 0
    off = int(ddesc[0, 0])
    for d in (d0, d1):
        dict_t[off:off + 500].copy_(torch.frombuffer(bytearray(d), dtype=torch.uint8))
        out.fill_(SENT)
        res.fill_(-1)
        st.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        outb = out.cpu().numpy()
        results = res.cpu().numpy()[:4 * n].view(np.uint8).reshape(-1).view(D.ERESULT_DTYPE)
        rec = D.EBatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
        tail = np.full(64, SENT, dtype=np.uint8)
        _verify(bufs, [d], None, opts, np.concatenate((outb, tail)), results, rec, "replay")


def test_the_dictionary_is_used(enc):
    """the golden text: its first 32 KiB as the dictionary, its next six 4 KiB pages as the buffers,
    K = 7 lazy.  Every FDICT stream is shorter than the old entry's stream of the same page; the oracle
    gives 10 340 bytes against 11 948 in total (the 4 DICTID bytes counted)"""
    bee = open(os.path.join(REPO, "tests", "golden", "bee_movie_script.txt"), "rb").read()
    d = bee[:32768]
    pages = [bee[32768 + 4096 * k:32768 + 4096 * (k + 1)] for k in range(6)]
    assert all(len(p) == 4096 for p in pages)
    opts = D.Opts(32768, 7, Z | DICT | FD | D.DMX_F_LAZY, 0)
    outb, results, rec = _run_and_verify(enc, pages, [d], None, opts)
    out, offsets, plain = D.compress_batch(pages, max_chain=7, lazy=True)
    assert all(int(a["out_len"]) < int(b["out_len"]) for a, b in zip(results, plain))
    assert (int(rec.out_len), int(plain["out_len"].sum())) == (10340, 11948)
    # the same through compress_batch(zdict=)
    out2, offsets2, res2 = D.compress_batch(pages, max_chain=7, lazy=True, zdict=d)
    assert out2.cpu().numpy().tobytes() == outb[:rec.out_len].tobytes() and res2.tobytes() == results.tobytes()
    back, boffs, bres = D.inflate_batch(out2, np.stack([res2["out_off"], res2["out_len"]], axis=1).astype(np.int64), zdict=d)
    assert back.cpu().numpy().tobytes() == b"".join(pages)


def test_compress_batch_python(enc):
    """compress_batch(zdict=, dict_of=, fdict=): a list of dictionaries, raw framing, a caller's encoder;
    without zdict the old entry, which still refuses the dictionary flags"""
    dicts = [_pre(300, 1), _pre(1024, 2)]
    bufs = [_buf(n, 70 + k) for k, n in enumerate([600, 2500, 0, 1024])]
    of = [1, None, 0, 0]
    for fmt, fdict, fl in (("zlib", True, Z | DICT | FD), ("zlib", False, Z | DICT), ("raw", True, RAW | DICT)):
        out, offsets, results = D.compress_batch(bufs, fmt=fmt, sw=1024, max_chain=7, lazy=True, zdict=dicts, dict_of=of,
                                                 fdict=fdict, encoder=enc)
        offs, flat = offsets.cpu().numpy(), out.cpu().numpy().tobytes()
        opts = D.Opts(1024, 7, fl | D.DMX_F_LAZY, 0)
        for k, b in enumerate(bufs):
            assert flat[offs[k]:offs[k + 1]] == _single(b, None if of[k] is None else dicts[of[k]], opts), (fmt, fdict, k)
    with pytest.raises(D.DeflateError) as ei:
        D.compress_batch(bufs, flags=FD)
    assert ei.value.code == -E["E_INVAL"]
    with pytest.raises(D.DeflateError) as ei:   # a dictionary index at or above the number of dictionaries
        D.compress_batch(bufs, sw=1024, zdict=dicts, dict_of=[0, 1, 2, 0])
    assert ei.value.code == -E["E_RANGE"]


def test_old_entries_before_and_after(enc):
    """one batch through dmx_encode_batch_async and one single dictionary encode on the same context
    give the same bytes before and after a dictionary batch"""
    bufs = [_buf(n, 80 + k) for k, n in enumerate([600, 2500, 0, 1024, 3077])]
    text, pre = _buf(100000, 5), _pre(2000, 5)

    def old():
        out, offsets, results = D.compress_batch(bufs, sw=1024, max_chain=7, lazy=True, encoder=enc)
        z, r = enc.compress_bytes(text, sw=32768, max_chain=7, flags=Z | DICT | FD | D.DMX_F_LAZY, pre=pre)
        assert r.status == 0
        return out.cpu().numpy().tobytes(), results.tobytes(), z, r.nblocks

    before = old()
    assert zlib.decompressobj(zdict=pre).decompress(before[2]) == text
    _run_and_verify(enc, bufs, [_pre(300)], None, D.Opts(1024, 7, Z | DICT | FD | D.DMX_F_LAZY, 0))
    assert old() == before
    assert D.lib().dmx_encode_batch_async(enc._ctx, None, 0, None, 0, 0, ctypes.byref(D.Opts(1024, 7, Z | DICT, 0)),
                                          ctypes.c_void_p(16), 0, ctypes.c_void_p(16), ctypes.c_void_p(16),
                                          None) == -E["E_INVAL"]
