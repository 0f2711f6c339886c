"""Batched range reads from BGZF files in device memory on the MI355X (dmx_bgzf_read_ranges_async,
dmx_bgzf_read_device; bgzf_read_ranges, bgzf_pread).  zlib / gzip are the judge: the bytes of range q
are data[off : off + len] of the decompressed file, the offsets their running sum, nmembers the
members Python finds touched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
from bgzf_ranges_inputs import named_file, want_bytes, want_members
from bgzf_read_inputs import bgzf_file

pytestmark = pytest.mark.gpu

E = D.E
SZ, RANGE, CRC, INVAL = -E["E_SZ"], -E["E_RANGE"], -E["E_CRC"], -E["E_INVAL"]
CANARY = 0xA5


@functools.lru_cache(maxsize=None)
def _text(n: int, seed: int = 61) -> bytes:
    return D.gen_text(max(n, 1), seed).tobytes()[:n]


def _dev(b: bytes, head: int = 0):
    """b as a CUDA tensor, `head` bytes into its storage"""
    t = torch.zeros(head + len(b), dtype=torch.uint8, device="cuda")
    if b:
        t[head:].copy_(torch.from_numpy(np.frombuffer(b, np.uint8).copy()))
    return t[head:]


def _check(data: bytes, lay, ranges, out, offsets, info=None):
    want = want_bytes(data, ranges)
    offs = offsets.cpu().numpy()
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    got = out.cpu().numpy().tobytes()
    assert len(got) == offs[-1]
    for q, w in enumerate(want):
        assert got[offs[q]:offs[q + 1]] == w, (q, ranges[q])
    if info is not None:
        assert info["nmembers"] == want_members(lay, data, ranges)
        assert info["out_len"] == len(got)


def _read(zt, data, lay, ranges, index=None, **kw):
    info = {}
    out, offsets = D.bgzf_read_ranges(zt, np.array(ranges, dtype=np.uint64).reshape(-1, 2), index=index, info=info, **kw)
    _check(data, lay, ranges, out, offsets, info)
    return info


class Call:
    """one dmx_bgzf_read_ranges_async call on buffers of its own: d_out lies `head` bytes into a
    buffer of CANARY bytes with 64 more behind it"""

    def __init__(self, zt, index, nranges: int, max_members: int, scratch: int, out_cap: int, head: int = 0,
                 verify: bool = True, flags: int = 0):
        self.zt, (self.ix, self.crcs, self.nblk, _) = zt, index
        self.n, self.mm, self.scratch, self.cap, self.head, self.flags = nranges, max_members, scratch, out_cap, head, flags
        self.want = self.crcs if verify else None
        self.ranges = torch.zeros((max(nranges, 1), 2), dtype=torch.int64, device="cuda")
        self.buf = torch.full((head + out_cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
        self.offsets = torch.full((nranges + 1,), -1, dtype=torch.int64, device="cuda")
        self.work = torch.zeros(int(D.lib().dmx_bgzf_ranges_work(self.nblk, nranges, max_members, scratch)), dtype=torch.uint8,
                                device="cuda")
        self.st = torch.full((32,), 0xEE, dtype=torch.uint8, device="cuda")
        assert self.work.data_ptr() % 256 == 0 and self.buf.data_ptr() % 16 == 0

    def set(self, ranges):
        a = np.array(ranges, dtype=np.uint64).reshape(-1, 2)
        assert len(a) == self.n
        self.ranges[:self.n].copy_(torch.from_numpy(a.view(np.int64)))

    def enqueue(self) -> int:
        return D.bgzf_read_ranges_async(self.zt, self.ix, self.want, self.nblk, self.ranges, self.n, self.flags,
                                        self.buf[self.head:self.head + self.cap], self.cap, self.offsets, self.mm, self.scratch,
                                        self.work, self.st)

    def record(self) -> D.RangesStatus:
        return D.RangesStatus.from_buffer_copy(self.st.cpu().numpy().tobytes())

    def out(self, n: int):
        return self.buf[self.head:self.head + n]

    def canaries(self, written: int) -> bool:
        b = self.buf.cpu().numpy()
        return bool((b[:self.head] == CANARY).all() and (b[self.head + written:] == CANARY).all())


def _plan(zt, index, ranges, flags: int = 0) -> D.RangesStatus:
    """the record of a call with all three capacities 0"""
    c = Call(zt, index, len(ranges), 0, 0, 0, flags=flags)
    c.set(ranges)
    assert c.enqueue() == 0
    return c.record()


# ---- 1. every range of a tiny file ----

def test_every_range_of_a_tiny_file():
    sizes = [3, 1, 0, 5, 2, 4]
    data = _text(15, 1)
    z, lay = bgzf_file(data, sizes, 6)
    zt = _dev(z)
    ranges = [(off, ln) for off in range(16) for ln in range(18)]
    ranges += [(15, 1), (16, 1), (1 << 40, 1), (0, 1 << 63), (7, 1 << 63), (15, 1 << 63), (16, 1 << 63), (1 << 40, 1 << 63),
               (1 << 63, 1 << 63), ((1 << 64) - 1, (1 << 64) - 1)]
    info = _read(zt, data, lay, ranges)
    assert info["nmembers"] == 5 and info["scratch_len"] == 15
    for r in ((0, 3), (3, 1), (4, 1), (2, 3), (14, 9), (15, 9), (0, 0)):   # and a few one by one
        got = D.bgzf_pread(zt, r[0], r[1])
        assert got.cpu().numpy().tobytes() == data[r[0]:r[0] + r[1]]
    # no ranges, and a file of empty members only
    out, offsets = D.bgzf_read_ranges(zt, np.zeros((0, 2), dtype=np.uint64))
    assert out.numel() == 0 and offsets.cpu().tolist() == [0]
    ze, laye = bgzf_file(b"", [0, 0], 6)
    _read(_dev(ze), b"", laye, [(0, 5), (3, 0)])
    assert D.bgzf_pread(_dev(ze), 0, 100).numel() == 0


# ---- 2. mixed real sizes ----

def test_mixed_real_sizes():
    sizes = [1, 65536, 0, 65280, 7, 0, 32768, 1000]
    data = _text(sum(sizes), 2)
    z, lay = bgzf_file(data, sizes, 6)
    zt = _dev(z)
    index = D.bgzf_index_gpu(zt)
    total = len(data)
    ranges = []
    for _, _, o, n in lay:
        b = o + n   # the end of this member: the boundary to the next one with data (empty ones lie on it)
        ranges += [(max(b - 1, 0), 1), (min(b, total - 1), 1), (max(b - 1, 0), 2), (max(b - 100, 0), 100), (b, 100)]
    ranges += [(0, total), (0, total), (5, 70000), (60000, 80000), (1, 65536), (65537, 65280), (total - 1000, 5000)]
    ranges += ranges[::-1]
    info = _read(zt, data, lay, ranges, index=index)
    assert info["nmembers"] == 6 and info["scratch_len"] == total
    out, offsets = D.bgzf_read_ranges(zt, np.array([[0, 1 << 62]], dtype=np.uint64), index=index)
    assert torch.equal(out, D.inflate_bgzf_tensor(zt)) and offsets.cpu().tolist() == [0, total]
    assert torch.equal(D.bgzf_pread(zt, 65530, 70000, index=index), out[65530:135530])


# ---- 3. alignment ----

def test_every_source_and_destination_alignment():
    data = _text(8192, 3)
    z, lay = bgzf_file(data, [4096, 4096], 6)
    zt = _dev(z, head=1)
    assert zt.data_ptr() % 16 == 1
    index = D.bgzf_index_gpu(zt)
    # range k: source offset = k // 16 mod 16; its destination follows from the lengths before it, which
    # are chosen so that it is (5 k + k // 16) mod 16 -- every residue once in each sixteen
    dest = [(5 * k + k // 16) % 16 for k in range(257)]
    ranges, at = [], 0
    for k in range(256):
        ln = (dest[k + 1] - dest[k]) % 16 + 16 * (k % 3)
        ln = 16 if ln == 0 else ln - 16 if ln > 40 else ln
        assert at % 16 == dest[k] and 1 <= ln <= 40
        ranges.append((16 * ((7 * k) % 400) + k // 16, ln))
        at += ln
    assert len({(off % 16, d) for (off, _), d in zip(ranges, dest)}) == 256
    for k in (200, 100, 10):   # lengths of 0 move nothing
        ranges.insert(k, (k, 0))
    need = _plan(zt, index, ranges)
    assert (need.status, need.nmembers, need.scratch_len, need.out_len) == (SZ, 2, 8192, at)
    for head in (1, 15, 0):
        c = Call(zt, index, len(ranges), 2, 8192, at, head=head)
        c.set(ranges)
        assert c.enqueue() == 0
        rec = c.record()
        assert (rec.status, rec.nmembers, rec.out_len) == (0, 2, at)
        _check(data, lay, ranges, c.out(at), c.offsets)
        assert c.canaries(at)


# ---- 4. tile edges ----

def test_scan_tile_edges():
    T, R = D.ranges_geometry()
    sizes = [1 + (k * 7) % 3 for k in range(T + 3)]
    data = _text(sum(sizes), 4)
    z, lay = bgzf_file(data, sizes, 1)
    zt = _dev(z)
    index = D.bgzf_index_gpu(zt)
    assert index[2] == T + 3
    o = [l[2] for l in lay] + [len(data)]
    # single members on both sides of the edge, alone and together; pairs and triples across it
    for ranges in ([(o[T - 1], 1)], [(o[T], 1)], [(o[T + 1], 1)], [(o[T + 2], 1)], [(o[T] - 1, 2)], [(o[T - 1], o[T + 2] - o[T - 1])],
                   [(o[T + 1] - 1, 2), (o[T - 2], 1)], [(o[T + 2], 9), (o[0], 1)], [(0, len(data))],
                   [(o[k], 1) for k in range(0, T + 3, 2)], [(o[k], 1) for k in (T + 2, T, T - 1, 1)]):
        _read(zt, data, lay, ranges, index=index)
    # R + 3 ranges: the offsets cross the range tile, lengths 0..3
    ranges = [((k * 3) % len(data), k % 4) for k in range(R + 3)]
    _read(zt, data, lay, ranges, index=index)
    ranges = [(o[T + 1], 1)] * (R - 1) + [(o[T] - 1, 3), (0, 0), (1, 1), (o[T + 2], 5)]
    _read(zt, data, lay, ranges, index=index)


# ---- 5. only what is asked ----

def test_only_the_touched_members_are_read():
    sizes = [500] * 40
    data = _text(sum(sizes), 5)
    z, lay = bgzf_file(data, sizes, 6)
    zb = bytearray(z)
    zb[lay[7][0] + lay[7][1] - 8] ^= 0x40      # member 7: its stored CRC-32
    zb[lay[23][0] + 18] = 0x07                 # member 23: BFINAL with BTYPE 3
    zt = _dev(bytes(zb))
    index = D.bgzf_index_gpu(zt)
    clean = [(k * 500 + 3, 400) for k in range(40) if k not in (7, 23)] + [(8 * 500, 15 * 500), (24 * 500, 8000)]
    assert _read(zt, data, lay, clean, index=index)["nmembers"] == 38
    assert _read(zt, data, lay, [(9 * 500 + k, 7) for k in range(50)], index=index)["nmembers"] == 1
    assert _read(zt, data, lay, [(9 * 500 - 1, 2)] * 50, index=index)["nmembers"] == 2
    with pytest.raises(D.DeflateError) as e:
        D.bgzf_read_ranges(zt, np.array([[0, 10], [7 * 500 + 499, 1]], dtype=np.uint64), index=index)
    assert e.value.code == CRC
    _read(zt, data, lay, [(0, 10), (7 * 500 + 499, 1), (3000, 1500)], index=index, verify=False)
    with pytest.raises(D.DeflateError) as whole:   # the decode's status: what the whole-file decode reports
        D.inflate_bgzf_tensor(zt, verify=False)
    assert whole.value.code == -E["E_ZBTYPE"]
    for verify in (True, False):
        with pytest.raises(D.DeflateError) as e:
            D.bgzf_read_ranges(zt, np.array([[23 * 500, 1], [0, 10]], dtype=np.uint64), index=index, verify=verify)
        assert e.value.code == whole.value.code
    with pytest.raises(D.DeflateError) as e:
        D.bgzf_pread(zt, 7 * 500 - 5, 10, index=index)
    assert e.value.code == CRC
    assert D.bgzf_pread(zt, 7 * 500 - 5, 10, index=index, verify=False).cpu().numpy().tobytes() == data[3495:3505]
    # a failed call leaves d_out alone
    c = Call(zt, index, 2, 2, 1000, 20)
    c.set([(0, 10), (7 * 500, 10)])
    assert c.enqueue() == 0
    assert c.record().status == CRC and c.canaries(0)


# ---- 6. capacities ----

def test_capacities_one_below_need():
    sizes = [300, 5000, 0, 70, 65536, 1200]
    data = _text(sum(sizes), 6)
    z, lay = bgzf_file(data, sizes, 6)
    zt = _dev(z)
    index = D.bgzf_index_gpu(zt)
    ranges = [(100, 300), (5300, 10), (5400, 1000), (70000, 0), (100, 300)]
    M, S, O = 4, 300 + 5000 + 70 + 65536, 300 + 10 + 1000 + 300
    need = _plan(zt, index, ranges)
    assert (need.status, need.nmembers, need.scratch_len, need.out_len, need.bad) == (SZ, M, S, O, 0xFFFFFFFF)
    for dm, ds, do in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        c = Call(zt, index, len(ranges), M - dm, S - ds, O - do)
        c.set(ranges)
        assert c.enqueue() == 0
        rec = c.record()
        assert (rec.status, rec.nmembers, rec.scratch_len, rec.out_len) == (SZ, M, S, O)
        assert c.canaries(0)
        assert c.offsets.cpu().tolist() == [0, 300, 310, 1310, 1310, 1610]
        c2 = Call(zt, index, len(ranges), rec.nmembers, rec.scratch_len, rec.out_len)
        c2.set(ranges)
        assert c2.enqueue() == 0
        assert c2.record().status == 0 and c2.canaries(O)
        _check(data, lay, ranges, c2.out(O), c2.offsets)


# ---- 7. virtual offsets ----

@pytest.mark.parametrize("named", [False, True])
def test_virtual_offsets(named):
    sizes = [700, 0, 65280, 3, 0, 0, 1500]
    data = _text(sum(sizes), 7)
    z, lay = (named_file if named else bgzf_file)(data, sizes, 6)
    zt = _dev(z)
    index = D.bgzf_index_gpu(zt)
    assert index[2] == 4
    vo = D.bgzf_voffset
    vr, lin = [], []
    for p, _, o, n in lay:
        if not n:
            continue
        for within, ln in ((0, 1), (n // 2, 1), (n - 1, 1), (n - 1, 2), (0, n + 5), (n // 2, 70000), (n - 1, 1 << 63), (n, 0), (0, 0)):
            vr.append((vo(p, within), ln))
            lin.append((o + within, ln))
    info = {}
    out, offsets = D.bgzf_read_ranges(zt, np.array(vr, dtype=np.uint64), index=index, virtual=True, info=info)
    _check(data, lay, lin, out, offsets, info)
    good = (vo(lay[0][0], 5), 10)
    bads = {"one past a member start": (vo(lay[2][0] + 1, 0), 1), "an empty member": (vo(lay[1][0], 0), 1),
            "the end-of-file member": (vo(lay[-1][0] + lay[-1][1], 0), 1), "within == ISIZE": (vo(lay[3][0], 3), 1),
            "past the file": (vo(len(z) + 100, 0), 0), "an empty member, len 0": (vo(lay[4][0], 0), 0)}
    for what, bad in bads.items():
        batch = [good] * 5 + [bad] + [good] * 3 + [bads["within == ISIZE"]] + [good]
        with pytest.raises(D.DeflateError) as e:
            D.bgzf_read_ranges(zt, np.array(batch, dtype=np.uint64), index=index, virtual=True)
        assert e.value.code == RANGE and "range 5 " in str(e.value), what
        c = Call(zt, index, len(batch), 4, len(data), 1000, flags=D.DMX_RANGES_VIRTUAL)
        c.set(batch)
        assert c.enqueue() == 0
        rec = c.record()
        assert (rec.status, rec.bad) == (RANGE, 5) and c.canaries(0), what
    with pytest.raises(D.DeflateError) as e:   # the same numbers are no error as plain offsets
        D.bgzf_read_ranges(zt, np.array([good, bads["within == ISIZE"]], dtype=np.uint64), index=index, virtual=True)
    assert "range 1 " in str(e.value)
    D.bgzf_read_ranges(zt, np.array([good, bads["within == ISIZE"]], dtype=np.uint64), index=index)


# ---- 8. index validation ----

def test_a_broken_index_is_refused():
    sizes = [100, 200, 300, 400]
    data = _text(sum(sizes), 8)
    z, lay = bgzf_file(data, sizes, 6)
    zt = _dev(z)
    ix, crcs, nblk, total = D.bgzf_index_gpu(zt)
    ranges = [(0, 50), (500, 100)]
    for entry, field, value in ((2, 1, 301), (1, 1, 99), (3, 2, 0), (0, 2, 65537), (0, 1, 1)):
        a = ix.cpu().numpy().copy().view(np.uint64).reshape(-1, 3)
        a[entry, field] = value
        broken = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
        c = Call(zt, (broken, crcs, nblk, total), len(ranges), nblk, total, 150)
        c.set(ranges)
        assert c.enqueue() == 0
        rec = c.record()
        assert rec.status == INVAL and c.canaries(0), (entry, field, value)
        assert c.offsets.cpu().tolist() == [-1, -1, -1]
    c = Call(zt, (ix, crcs, nblk, total), len(ranges), nblk, total, 150)   # and the index as it was
    c.set(ranges)
    assert c.enqueue() == 0 and c.record().status == 0
    _check(data, lay, ranges, c.out(150), c.offsets)


# ---- 9. the encoder's output, in place ----

def test_ranges_of_the_encoders_own_output():
    data = _text(200_000, 9)
    enc = D.Encoder(0, len(data))
    try:
        zt, r = enc.compress_tensor(_dev(data), opts=D.Opts(32768, 8, D.DMX_BGZF, 0))
        assert r.status == 0
        index = D.bgzf_index_gpu(zt)
        assert index[2] == 7 and index[3] == len(data)
        rng = np.random.default_rng(9)
        ranges = [(int(rng.integers(0, len(data))), int(rng.integers(0, 40_000))) for _ in range(100)]
        lay = [(0, 0, 32768 * k, min(32768, len(data) - 32768 * k)) for k in range(7)]
        _read(zt, data, lay, ranges, index=index)
    finally:
        enc.close()


# ---- 10. graph capture ----

def test_ranges_in_a_graph():
    """the async call captured once on a side stream -- kernels only, one after the other -- and
    replayed while the ranges change on the device: other ranges, then a batch that needs more
    members than max_members, then the first again"""
    sizes = [1000] * 12
    data = _text(sum(sizes), 10)
    z, lay = bgzf_file(data, sizes, 6)
    zt = _dev(z)
    index = D.bgzf_index_gpu(zt)
    a = [(10, 100), (1990, 20), (5000, 0), (11_999, 50)]
    b = [(7000, 1500), (0, 1), (7100, 10), (3000, 3)]
    over = [(0, 2500), (4000, 1), (6000, 1), (8000, 1)]     # 6 members
    c = Call(zt, index, 4, 5, 5000, 2000)
    c.set(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the kernels are loaded before the capture
        assert c.enqueue() == 0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r = c.enqueue()
    assert r == 0
    for ranges in (a, b, over, a):
        c.set(ranges)
        c.buf.fill_(CANARY)
        c.st.fill_(0xEE)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        rec = c.record()
        if ranges is over:
            assert (rec.status, rec.nmembers, rec.scratch_len, rec.out_len) == (SZ, 6, 6000, 2503) and c.canaries(0)
            assert c.offsets.cpu().tolist() == [0, 2500, 2501, 2502, 2503]
            continue
        n = sum(len(w) for w in want_bytes(data, ranges))
        assert (rec.status, rec.nmembers, rec.out_len) == (0, want_members(lay, data, ranges), n)
        _check(data, lay, ranges, c.out(n), c.offsets)
        assert c.canaries(n)
