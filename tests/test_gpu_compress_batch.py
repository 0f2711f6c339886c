"""Batches of independent buffers into independent streams on the GPU (dmx_encode_batch_async,
compress_batch): every stream's bytes are what a single encode of its buffer gives with the same
options -- which is the specification, and puts every stream under the oracle the single encode is
pinned to -- at every input alignment, across the scan's tile edges in both launch shapes of K3,
with void table entries, at the capacities' edges, with bad streams among good ones, for
degenerate batches, in a captured graph, and round-tripped through inflate_batch."""
import gzip
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D

pytestmark = pytest.mark.gpu

E = D.E
FMT = {"zlib": D.DMX_ZLIB, "gzip": D.DMX_GZIP, "raw": D.DMX_F_FINAL}
SENT = 0xA5


def _host_inflate(fmt, z):
    if fmt == "zlib":
        return zlib.decompress(z)
    if fmt == "gzip":
        return gzip.decompress(z)
    d = zlib.decompressobj(-15)
    out = d.decompress(z) + d.flush()
    assert d.eof and not d.unused_data
    return out


def _check_of(fmt, data):
    return zlib.adler32(data) if fmt == "zlib" else zlib.crc32(data) if fmt == "gzip" else 0


_TEXT = D.gen_text(1 << 18, 7).tobytes()
_RAND = D.gen_random(1 << 18, 11).tobytes()


def _content(kind, n, salt):
    o = (salt * 7919) % 50000
    if kind == "text":
        return _TEXT[o:o + n]
    if kind == "random":
        return _RAND[o:o + n]
    if kind == "zeros":
        return bytes(n)
    a, b = n // 3, 2 * n // 3   # a mix: text, random bytes, zeros
    return _TEXT[o:o + a] + _RAND[o:o + b - a] + bytes(n - b)


def _lay(bufs, residues=True):
    """the buffers in one tensor with gaps of 0..17 junk bytes; with `residues` buffer k starts at an
    address that is k mod 16 (the gap that gets there is 0..15)"""
    parts, desc, cur = [], [], 0
    for k, b in enumerate(bufs):
        gap = (k - cur) % 16 if residues else (5 * k) % 18
        parts.append(bytes([0xEE]) * gap)
        cur += gap
        desc.append((cur, len(b)))
        parts.append(b)
        cur += len(b)
    parts.append(bytes([0xEE]) * 17)
    t = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, np.array(desc, dtype=np.int64).reshape(-1, 2)


def _blocks(desc, sw):
    return D.encode_batch_blocks(desc[:, 1].tolist(), sw)


def _batch(enc, t, desc, opts, max_blocks=None, out_cap=None, out=None, expect_rc=0):
    """one dmx_encode_batch_async call on a sentinel-filled output; returns (out bytes, results, record)"""
    L = D.lib()
    n = desc.shape[0]
    sw = opts.sw or 32768
    if max_blocks is None:
        max_blocks = _blocks(desc, sw)
    cap = int(L.dmx_encode_batch_bound(int(desc[:, 1].clip(0, t.numel()).sum()), n, sw, opts.flags))
    if out is None:
        out = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    if out_cap is None:
        out_cap = cap
    enc.reserve_batch(max_blocks, n, sw, opts.flags)
    dt = torch.from_numpy(np.ascontiguousarray(desc)).cuda() if n else torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    res = torch.full((max(n, 1) * 4,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()   # (on the default stream the call runs on the encoder's own stream)
    rc = D.compress_batch_async(enc, t, dt, n, max_blocks, out, out_cap, res, st, opts)
    assert rc == expect_rc, rc
    torch.cuda.synchronize()
    results = res.cpu().numpy()[:4 * n].view(np.uint8).reshape(-1).view(D.ERESULT_DTYPE)
    rec = D.EBatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    return out.cpu().numpy(), results, rec


def _singles(enc, t, desc, opts):
    """the specification: Encoder.compress_tensor of every buffer alone (where it lies: same alignment)"""
    zs = []
    for off, ln in desc.tolist():
        z, r = enc.compress_tensor(t[off:off + ln], opts=opts)
        assert r.status == 0
        zs.append(z.cpu().numpy().tobytes())
    return zs


def _verify(fmt, bufs, singles, outb, results, rec, what=""):
    pos = 0
    for k, (data, want) in enumerate(zip(bufs, singles)):
        r = results[k]
        assert r["status"] == 0, (what, k, r)
        assert int(r["out_off"]) == pos, (what, k, int(r["out_off"]), pos)
        got = outb[pos:pos + int(r["out_len"])].tobytes()
        assert got == want, (what, k, len(data), len(got), len(want))
        assert _host_inflate(fmt, got) == data, (what, k)
        assert int(r["check"]) == _check_of(fmt, data), (what, k)
        pos += int(r["out_len"])
    assert rec.status == 0 and rec.nfailed == 0 and rec.first_bad == 0xFFFFFFFF, (what, rec.status, rec.nfailed)
    assert rec.out_len == pos, (what, rec.out_len, pos)
    assert rec.in_len == sum(len(b) for b in bufs)
    tail = (pos + 3) & ~3
    assert (outb[tail:] == SENT).all(), (what, "a byte at or beyond align4(out_len) was written")


OPTSETS = {
    "exhaustive": (0, 0),
    "bench_default": (7, D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK),
    "k4_greedy": (4, 0),
    "exact_sort": (7, D.DMX_F_EXACT_SORT),
}
LENS_1K = [0, 1, 2, 3, 4, 1023, 1024, 1025, 2048, 2049, 3089]


@pytest.fixture(scope="module")
def enc():
    e = D.Encoder(0, 1 << 20)
    yield e
    e.close()


@pytest.fixture(scope="module")
def parity_input():
    bufs = [_content(kind, n, 13 * i + j) for i, kind in enumerate(("text", "random", "zeros", "mix"))
            for j, n in enumerate(LENS_1K)]
    t, desc = _lay(bufs)
    assert {(t.data_ptr() + int(o)) % 16 for o in desc[:, 0]} == set(range(16))
    return bufs, t, desc


@pytest.mark.parametrize("fmt", sorted(FMT))
@pytest.mark.parametrize("optset", sorted(OPTSETS))
def test_parity_with_single_encodes(enc, parity_input, fmt, optset):
    """sw = 1024, lengths around every block edge, four kinds of content, every address residue mod
    16: the batch's streams are the single encodes' bytes, inflate on the host, and carry their check"""
    bufs, t, desc = parity_input
    k, fl = OPTSETS[optset]
    opts = D.Opts(1024, k, FMT[fmt] | fl, 0)
    outb, results, rec = _batch(enc, t, desc, opts)
    r = enc.result()   # dmx_encode_result after a batch: the totals
    _verify(fmt, bufs, _singles(enc, t, desc, opts), outb, results, rec, f"{fmt}/{optset}")
    assert rec.nblocks == _blocks(desc, 1024) == sum(int(x["nblocks"]) for x in results)
    assert (r.out_len, r.n, r.adler, r.status) == (rec.out_len, rec.in_len, 0, 0)
    assert r.nblocks == rec.nblocks == r.nstored + r.nfixed + r.ndynamic


@pytest.mark.parametrize("fmt", sorted(FMT))
def test_parity_full_blocks_store_check(enc, fmt):
    """sw = 32768 around the full block, text and random bytes under the store check (the noise
    blocks are stored by K0, without its speculative copy)"""
    lens = [1, 32767, 32768, 32769, 65541]
    bufs = [_content(kind, n, 3 + j) for kind in ("text", "random") for j, n in enumerate(lens)]
    t, desc = _lay(bufs)
    opts = D.Opts(32768, 7, FMT[fmt] | D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK, 0)
    outb, results, rec = _batch(enc, t, desc, opts)
    assert enc.result().nstored >= 5   # the random buffers' blocks of 32767 and 32768 bytes: 1 + 1 + 1 + 2
    _verify(fmt, bufs, _singles(enc, t, desc, opts), outb, results, rec, fmt)


@pytest.fixture(scope="module")
def tiles_input():
    """sw = 64, 700 streams of 1, 2, 3 blocks in turn (k % 3 + 1): stream k starts at block
    6 (k // 3) + (0, 1, 3)[k % 3], 1 400 blocks, six scan tiles.  Block 255 = 6 * 42 + 3 is the first
    block of stream 128 (three blocks: 255, 256, 257), so that one is moved: stream 127 (two blocks,
    253 and 254) is made three blocks long and stream 128 two -- then stream 127 ends with block 255,
    and a stream boundary lies exactly at 255 | 256 (streams 127 | 128).  Blocks 510 = 6 * 85 .. are
    stream 255 (one block: 510), stream 256 (two: 511, 512): stream 256 spans 511 | 512."""
    lens = []
    for k in range(700):
        nb = k % 3 + 1
        if k == 127:
            nb = 3
        if k == 128:
            nb = 2
        lens.append(64 * nb - (k % 5))   # the last block is 60..64 bytes
    bufs = [_content(("text", "zeros", "random", "mix")[k % 4], n, k) for k, n in enumerate(lens)]
    t, desc = _lay(bufs, residues=False)
    starts = np.concatenate(([0], np.cumsum([-(-n // 64) for n in lens])))
    assert starts[128] == 256 and starts[127] == 253           # a boundary at 255 | 256
    assert starts[256] == 511 and starts[257] == 513           # stream 256 spans 511 | 512
    assert starts[-1] > 512
    return bufs, t, desc


def test_tile_edges_both_scan_shapes(enc, tiles_input):
    bufs, t, desc = tiles_input
    opts = D.Opts(64, 7, D.DMX_ZLIB | D.DMX_F_LAZY, 0)
    singles = _singles(enc, t, desc, opts)
    runs = []
    try:
        for scan3 in (0, 1):
            enc.set_hook("scan3", scan3)
            outb, results, rec = _batch(enc, t, desc, opts)
            _verify("zlib", bufs, singles, outb, results, rec, f"scan3={scan3}")
            runs.append((outb.tobytes(), results.tobytes(), bytes(rec)))
    finally:
        enc.set_hook("scan3", 0)
    assert runs[0] == runs[1]


def test_void_blocks(enc, tiles_input):
    """max_blocks exact, exact + 1 and 2 x exact + 7: workgroups beyond the real count return at once"""
    bufs, t, desc = tiles_input
    bufs, desc = bufs[:300], desc[:300]
    opts = D.Opts(64, 4, D.DMX_GZIP, 0)
    exact = _blocks(desc, 64)
    runs = []
    for mb in (exact, exact + 1, 2 * exact + 7):
        outb, results, rec = _batch(enc, t, desc, opts, max_blocks=mb)
        assert rec.status == 0 and rec.nblocks == exact
        runs.append((outb.tobytes(), results.tobytes(), bytes(rec)))
    assert runs[0] == runs[1] == runs[2]
    _verify("gzip", bufs, _singles(enc, t, desc, opts), np.frombuffer(runs[0][0], dtype=np.uint8),
            np.frombuffer(runs[0][1], dtype=D.ERESULT_DTYPE), D.EBatchStatus.from_buffer_copy(runs[0][2]))


def test_capacities(enc, parity_input):
    bufs, t, desc = parity_input
    opts = D.Opts(1024, 7, D.DMX_ZLIB | D.DMX_F_LAZY, 0)
    exact = _blocks(desc, 1024)
    good, gres, grec = _batch(enc, t, desc, opts)
    assert grec.status == 0
    # one block short: -E_SZ, the record holds the need, no byte written
    outb, results, rec = _batch(enc, t, desc, opts, max_blocks=exact - 1)
    assert rec.status == -E["E_SZ"] and rec.nblocks == exact
    assert (outb == SENT).all()
    with pytest.raises(D.DeflateError) as ei:   # dmx_encode_result: the same status
        enc.result()
    assert ei.value.code == -E["E_SZ"]
    # out_cap = align4(out_len): succeeds, and nothing from there on is written
    a4 = (grec.out_len + 3) & ~3
    outb, results, rec = _batch(enc, t, desc, opts, out_cap=a4)
    assert rec.status == 0 and rec.out_len == grec.out_len
    assert outb[:rec.out_len].tobytes() == good[:rec.out_len].tobytes() and results.tobytes() == gres.tobytes()
    assert (outb[a4:] == SENT).all()
    # four bytes less: -E_SZ, out_len reported, the streams' places too, no byte written
    outb, results, rec = _batch(enc, t, desc, opts, out_cap=a4 - 4)
    assert rec.status == -E["E_SZ"] and rec.out_len == grec.out_len and rec.nblocks == exact
    assert (outb == SENT).all()
    assert (results["out_off"] == gres["out_off"]).all() and (results["out_len"] == gres["out_len"]).all()


def test_bad_streams(enc, parity_input):
    bufs, t, desc = parity_input
    bufs, desc = bufs[20:32], desc[20:32]
    opts = D.Opts(1024, 7, D.DMX_GZIP | D.DMX_F_LAZY, 0)
    good, gres, grec = _batch(enc, t, desc, opts)
    bad = np.insert(desc, [3, 9], [[t.numel() - 2, 3], [-8, 16]], axis=0)   # past the end; in_off + in_len wraps
    outb, results, rec = _batch(enc, t, bad, opts, max_blocks=_blocks(desc, 1024))
    assert rec.status == 0 and rec.nfailed == 2 and rec.first_bad == 3
    assert rec.out_len == grec.out_len and rec.in_len == grec.in_len and rec.nblocks == grec.nblocks
    assert outb[:rec.out_len].tobytes() == good[:grec.out_len].tobytes()
    for k in (3, 10):
        assert results[k]["status"] == -E["E_RANGE"] and results[k]["out_len"] == 0 and results[k]["nblocks"] == 0
    keep = np.delete(results, [3, 10])
    assert keep.tobytes() == gres.tobytes()
    offs = np.concatenate((results["out_off"], [rec.out_len])).astype(np.int64)
    assert (np.diff(offs) == results["out_len"].astype(np.int64)).all()


@pytest.mark.parametrize("fmt", sorted(FMT))
def test_degenerate_batches(enc, fmt):
    empty = {"zlib": bytes.fromhex("789c030000000001"), "raw": b"\x03\x00", "gzip": gzip.compress(b"")}[fmt]
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    opts = D.Opts(32768, 7, FMT[fmt], 0)
    outb, results, rec = _batch(enc, t, np.zeros((0, 2), dtype=np.int64), opts)
    assert (rec.status, rec.nfailed, rec.first_bad, rec.nblocks, rec.out_len, rec.in_len) == (0, 0, 0xFFFFFFFF, 0, 0, 0)
    assert (outb == SENT).all()
    desc = np.array([[0, 0], [64, 0], [7, 0]], dtype=np.int64)
    outb, results, rec = _batch(enc, t, desc, opts)
    assert rec.status == 0 and rec.nblocks == 3
    assert len(empty) == (20 if fmt == "gzip" else len(empty)) and _host_inflate(fmt, empty) == b""
    for k in range(3):
        z = outb[int(results[k]["out_off"]):][:int(results[k]["out_len"])].tobytes()
        assert _host_inflate(fmt, z) == b""
        assert z == enc.compress_tensor(t[:0], opts=opts)[0].cpu().numpy().tobytes()
        if fmt != "gzip":
            assert z == empty
        assert results[k]["check"] == _check_of(fmt, b"")
    assert rec.out_len == 3 * len(empty)


def test_context_afterwards(enc, parity_input):
    """a single encode on the same Encoder gives the same bytes and dmx_result before and after a
    batch; the block index of a batch is refused"""
    bufs, t, desc = parity_input
    text = torch.frombuffer(bytearray(_TEXT[:200000]), dtype=torch.uint8).cuda()
    o1 = D.Opts(32768, 7, D.DMX_ZLIB | D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK, 0)
    z0, r0 = enc.compress_tensor(text, opts=o1)
    z0 = z0.cpu().numpy().tobytes()
    _batch(enc, t, desc, D.Opts(1024, 7, D.DMX_GZIP | D.DMX_F_STORE_CHECK, 0))
    idx = torch.zeros(3 * 4096, dtype=torch.int64, device="cuda")
    assert D.lib().dmx_block_index(enc._ctx, idx.data_ptr(), 4096, None) == -E["E_INVAL"]
    z1, r1 = enc.compress_tensor(text, opts=o1)
    assert z1.cpu().numpy().tobytes() == z0 and zlib.decompress(z0) == _TEXT[:200000]
    skip = ("nsortfallback_total",)
    assert [getattr(r0, f) for f, _ in D.Result._fields_ if f not in skip] == \
           [getattr(r1, f) for f, _ in D.Result._fields_ if f not in skip]
    assert D.lib().dmx_block_index(enc._ctx, idx.data_ptr(), 4096, None) == r1.nblocks


def test_batch_in_a_graph(enc):
    """one call captured on a side stream -- kernels only, one after the other -- and replayed while
    the input bytes change in place: each replay equals the eager call on the same bytes"""
    lens = [3000, 0, 1024, 5000, 77]
    def fill(seed):
        return [_content(("text", "mix", "random")[(k + seed) % 3], n, 31 * seed + k) for k, n in enumerate(lens)]
    t, desc = _lay(fill(0), residues=False)
    opts = D.Opts(1024, 7, D.DMX_GZIP | D.DMX_F_LAZY, 0)
    n, mb = len(lens), _blocks(desc, 1024)
    cap = int(D.lib().dmx_encode_batch_bound(sum(lens), n, 1024, opts.flags))
    enc.reserve_batch(mb, n, 1024, opts.flags)
    dt = torch.from_numpy(desc).cuda()
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    res = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")

    def enqueue():
        return D.compress_batch_async(enc, t, dt, n, mb, out, cap, res, st, opts)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the kernels are loaded before the capture
        assert enqueue() == 0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r = enqueue()
    assert r == 0
    for seed in (1, 2):
        bufs = fill(seed)
        for (off, ln), b in zip(desc.tolist(), bufs):
            if ln:
                t[off:off + ln].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
        out.fill_(SENT)
        res.fill_(-1)
        st.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = (out.cpu().numpy().tobytes(), res.cpu().numpy().tobytes(), st.cpu().numpy().tobytes())
        outb, results, rec = _batch(enc, t, desc, opts)   # the eager call on the same bytes
        assert got[0][:rec.out_len] == outb[:rec.out_len].tobytes()
        assert got[1] == results.tobytes() and got[2] == bytes(rec)
        _verify("gzip", bufs, _singles(enc, t, desc, opts), outb, results, rec, f"replay {seed}")


@pytest.mark.parametrize("fmt", sorted(FMT))
def test_round_trip_on_the_device(fmt):
    """inflate_batch(compress_batch(bufs)) returns the buffers"""
    bufs = [_content(("text", "mix", "zeros", "random")[k % 4], n, k)
            for k, n in enumerate([0, 1, 5, 1000, 32768, 32769, 70000, 3, 0, 100000])]
    out, offsets, results = D.compress_batch(bufs, fmt=fmt, max_chain=7, lazy=True, flags=D.DMX_F_DEEP | D.DMX_F_STORE_CHECK)
    assert out.is_cuda and out.dtype == torch.uint8 and offsets.dtype == torch.int64 and offsets.numel() == len(bufs) + 1
    offs = offsets.cpu().numpy()
    assert offs[0] == 0 and offs[-1] == out.numel() and (np.diff(offs) == results["out_len"].astype(np.int64)).all()
    for k, b in enumerate(bufs):
        assert results[k]["check"] == _check_of(fmt, b)
    streams = np.stack([offs[:-1], np.diff(offs)], axis=1)
    back, boffs, bres = D.inflate_batch(out, streams, fmt=fmt)
    bo = boffs.cpu().numpy()
    flat = back.cpu().numpy().tobytes()
    for k, b in enumerate(bufs):
        assert flat[bo[k]:bo[k] + int(bres[k]["out_len"])] == b, k
    # the tensor form of the input, and a caller's encoder
    t, desc = _lay(bufs, residues=False)
    e = D.Encoder(0, 0)
    try:
        out2, offsets2, results2 = D.compress_batch(t, desc, fmt=fmt, max_chain=7, lazy=True,
                                                    flags=D.DMX_F_DEEP | D.DMX_F_STORE_CHECK, encoder=e)
    finally:
        e.close()
    assert results2.tobytes() == results.tobytes() and torch.equal(out2, out) and torch.equal(offsets2, offsets)
    with pytest.raises(D.DeflateError):
        D.compress_batch(t, [[t.numel(), 1]], fmt=fmt)
