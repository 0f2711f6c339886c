"""Reading any BGZF file on the MI355X: members of up to 65 536 bytes through
dmx_inflate_members_async (inflate_bgzf_gpu, decompress_bgzf), the CRC-32 of every member checked on
the device by the range kernel (crc32_ranges) whatever the mix of member sizes.  The files are made
with Python's zlib (tests/bgzf_read_inputs.py), which also judges them: every member is at most
65 536 bytes and gzip.decompress gives the data back."""
import ctypes
import functools
import gzip
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
import deflate_craft as C
from bgzf_read_inputs import EOF_MEMBER, HTS, TOP, bgzf_file, deflate_matches, entries, hts_sizes, member, wrap

pytestmark = pytest.mark.gpu

GUARD = 0x5A
E = D.E


@functools.lru_cache(maxsize=None)
def _text(n: int, seed: int = 31) -> bytes:
    return D.gen_text(max(n, 1), seed).tobytes()[:n]


@functools.lru_cache(maxsize=None)
def _noise(n: int, seed: int = 32) -> bytes:
    return D.gen_random(max(n, 1), seed).tobytes()[:n]


def _dev(b: bytes):
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()


def _members(z: bytes, idx: np.ndarray, crcs, out_ptr: int, out_cap: int, stream=None):
    """dmx_inflate_members_async on raw pointers: (return value, status, out_len)"""
    zt, ix = _dev(z), _dev(idx.tobytes())
    want = _dev(np.asarray(crcs, np.uint32).tobytes()) if crcs is not None else None
    st = torch.full((16,), 0xEE, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    r = D.lib().dmx_inflate_members_async(ctypes.c_void_p(zt.data_ptr()), zt.numel(), ctypes.c_void_p(ix.data_ptr()),
                                          idx.size // 24, ctypes.c_void_p(out_ptr), out_cap,
                                          ctypes.c_void_p(want.data_ptr() if want is not None else 0),
                                          ctypes.c_void_p(st.data_ptr()), ctypes.c_void_p(s))
    torch.cuda.synchronize()
    h = st.cpu().numpy()
    return r, int(h[:4].view(np.int32)[0]), int(h[8:16].view(np.uint64)[0])


def _code(f, *a, **kw) -> int:
    try:
        f(*a, **kw)
    except D.DeflateError as e:
        return e.code
    return 0


# ---- files as htslib writes them ----

@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_htslib_shaped_file(level):
    n = 200000
    data = _text(n)
    z, lay = bgzf_file(data, hts_sizes(n), level)
    assert [m[3] for m in lay] == [HTS, HTS, HTS, n - 3 * HTS]
    if level == 0:   # a stored DEFLATE block of more than 32 768 bytes inside a member
        assert z[18] & 6 == 0 and int.from_bytes(z[19:21], "little") > 32768
    assert _code(D.bgzf_index, z) == -E["E_RANGE"]   # out of range for the 32 KiB reader, as before
    assert D.inflate_bgzf_gpu(z).cpu().numpy().tobytes() == data
    assert D.inflate_bgzf_gpu(z, verify=False).cpu().numpy().tobytes() == data
    assert D.decompress_bgzf(z) == data
    assert D.decompress_bgzf(z, verify=False) == data


MIXED = [1234, HTS, TOP, 1, 0, 40000, 32768, 32769]


def test_mixed_member_sizes_verify():
    data = _text(sum(MIXED), 33)
    z, _ = bgzf_file(data, MIXED, 6)
    assert D.inflate_bgzf_gpu(z, verify=True).cpu().numpy().tobytes() == data
    assert D.decompress_bgzf(z, verify=True) == data
    # one wrong stored CRC among them is found (the short member behind the 65 536-byte one)
    idx, crcs, total = D.bgzf_index(z, 65536)
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    assert _members(z, idx, crcs, out.data_ptr(), total) == (0, 0, total)
    bad = crcs.copy()
    bad[3] ^= 1
    assert _members(z, idx, bad, out.data_ptr(), total) == (0, -E["E_CRC"], total)
    assert out.cpu().numpy().tobytes() == data


# ---- sources farther back than the ring, on both sides of position 32 768 ----

CHAIN = [8193, 8191, 8192, 8193, 8191, 8192]    # one slice of the noise, copied at these spacings
RUN = (31768, 33768)                             # a run of one byte over position 32 768 (4 rings)
SLICE = 300


@functools.lru_cache(maxsize=None)
def _far_member():
    """65 536 bytes for zlib level 9: 20 000 bytes of noise, text, a slice of the noise copied
    again and again at the spacings of CHAIN (zlib takes the nearest copy: those distances, from
    positions below and above 32 768) and a run of one byte over position 32 768"""
    b = bytearray(_noise(20000) + _text(TOP - 20000, 34))
    want = []   # (position, distance) of every copy
    p = 3000
    for d in CHAIN:
        b[p + d:p + d + SLICE] = b[p:p + SLICE]
        p += d
        want.append((p, d))
    b[RUN[0]:RUN[1]] = b"Z" * (RUN[1] - RUN[0])
    spans = sorted([(p, p + SLICE) for p, _ in want] + [RUN])
    assert all(a[1] <= c[0] for a, c in zip(spans, spans[1:])) and spans[0][0] >= 3000 + SLICE and spans[-1][1] <= TOP
    return bytes(b), want


@functools.lru_cache(maxsize=None)
def _longest_distance_member():
    """zlib never emits a distance above 32 768 - 262, so the distances 32 767 and 32 768 are
    written by hand (tests/deflate_craft.py): 34 000 stored bytes, then one fixed-code block of
    matches of 258 bytes at 32 767 and 32 768 in turn up to 65 536 bytes -- every one of them
    from an output position above 32 768.  Returns (data, raw DEFLATE)."""
    head = _noise(20000, 43) + _text(14000, 44)
    out, items, k = bytearray(head), [], 0
    while len(out) < TOP:
        ln, d = min(258, TOP - len(out)), (32767, 32768)[k % 2]
        items += C.match(ln, d)
        for _ in range(ln):
            out.append(out[-d])
        k += 1
    raw = C.Deflate().stored(head, False).fixed_block(items + [("L", 256)], True).getvalue()
    return bytes(out), raw


def test_far_sources_past_32k():
    data, want = _far_member()
    assert len(data) == TOP
    m = member(data, 9)
    # the stream really holds those distances, at positions below and above 32 768, and the run
    # of distance 1 crosses 32 768 and a ring boundary
    mt = deflate_matches(m[18:-8])
    for p, d in want:
        got = [(q, ln) for q, ln, dd in mt if dd == d and p <= q < p + SLICE]
        assert sum(ln for _, ln in got) >= SLICE - 8, (p, d, got)
    for d in (8191, 8192, 8193):
        assert any(p < 32768 for p, dd in want if dd == d) and any(p > 32768 for p, dd in want if dd == d)
    assert any(dd == 1 and ln == 258 and q < 32768 < q + ln for q, ln, dd in mt)
    assert any(dd == 1 and q // 8192 != (q + ln - 1) // 8192 for q, ln, dd in mt)
    data2, raw2 = _longest_distance_member()
    m2 = wrap(raw2, data2)
    mt2 = deflate_matches(raw2)
    assert len(data2) == TOP and len(mt2) == 123 and {dd for _, _, dd in mt2} == {32767, 32768}
    assert all(q >= 34000 for q, _, _ in mt2)
    z = m + m2 + EOF_MEMBER
    assert gzip.decompress(z) == data + data2
    assert D.inflate_bgzf_gpu(z).cpu().numpy().tobytes() == data + data2
    assert D.decompress_bgzf(z) == data + data2


# ---- an output that starts at an odd address ----

def test_output_at_an_odd_address():
    n = 2 * HTS + 4321
    data = _text(n, 35)
    z, _ = bgzf_file(data, hts_sizes(n), 6)
    idx, crcs, total = D.bgzf_index(z, 65536)
    big = torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda")
    for odd in (1, 15):
        big.fill_(GUARD)
        out = big[odd:odd + n]
        assert out.data_ptr() % 16 == odd
        assert _members(z, idx, crcs, out.data_ptr(), n) == (0, 0, n)
        h = big.cpu().numpy()
        assert h[odd:odd + n].tobytes() == data
        assert (h[:odd] == GUARD).all() and (h[odd + n:] == GUARD).all()


# ---- the range CRC ----

LENGTHS = [0, 1, 15, 16, 17, 32767, 32768, 32769, 65535, 65536]


def _ranges_raw(t, ent, st_init=0):
    """dmx_crc32_ranges_async on entries [(off, len)]: (return value, status, words)"""
    rec = np.zeros((len(ent), 3), np.uint64)
    for k, (off, ln) in enumerate(ent):
        rec[k] = (0xDEAD, off, ln)   # (bit is not read)
    ix = _dev(rec.tobytes())
    w = torch.full((len(ent) + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    st[0] = st_init
    r = D.lib().dmx_crc32_ranges_async(ctypes.c_void_p(t.data_ptr()), t.numel(), ctypes.c_void_p(ix.data_ptr()), len(ent),
                                       ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(st.data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    h = w.cpu().numpy().view(np.uint32)
    assert h[len(ent)] == 0x5A5A5A5A, "the word behind d_crc was written"
    return r, int(st[0].item()), h[:len(ent)].tolist()


@pytest.mark.parametrize("kind", ["random", "zeros", "ff"])
def test_crc32_ranges_vs_zlib(kind):
    n = 150001
    h = {"random": np.frombuffer(_noise(n, 36), np.uint8), "zeros": np.zeros(n, np.uint8), "ff": np.full(n, 0xFF, np.uint8)}[kind]
    hb = h.tobytes()
    base = torch.empty(n + 256 + 16, dtype=torch.uint8, device="cuda")
    a0 = (-base.data_ptr()) % 256   # a 256-byte aligned start inside the tensor
    rng = np.random.default_rng(37)
    for toff in (0, 3):
        t = base[a0 + toff:a0 + toff + n]
        t.copy_(torch.from_numpy(h.copy()))
        ent = []
        for ln in LENGTHS:
            for mod in (0, 1, 15):   # the range's address mod 16
                k = int(rng.integers(0, (n - ln - 32) // 16))
                ent.append((16 * k + (mod - toff) % 16, ln))
        ent.append((n - 65536, 65536))           # ends with the buffer
        ent.append((n - 1, 1))
        ent.append((n, 0))                       # empty, at the very end
        ent.append((70000, 30000))               # these two overlap
        ent.append((80000, 30000))
        order = rng.permutation(len(ent))        # out of order
        ent = [ent[i] for i in order]
        assert any(a[0] > b[0] for a, b in zip(ent, ent[1:]))
        want = [zlib.crc32(hb[o:o + ln]) for o, ln in ent]
        assert _ranges_raw(t, ent) == (0, 0, want), (kind, toff)
        ix = _dev(np.array([(0, o, ln) for o, ln in ent], np.uint64).tobytes())
        assert D.crc32_ranges(t, ix, len(ent)).cpu().numpy().view(np.uint32).tolist() == want
        # one entry past n and one of 65 537 bytes: -E_RANGE, their words untouched, the others right
        bad = list(ent)
        bad.insert(5, (n - 10, 11))
        bad.insert(20, (0, 65537))
        r, st, got = _ranges_raw(t, bad)
        wb = list(want)
        wb.insert(5, 0x5A5A5A5A)
        wb.insert(20, 0x5A5A5A5A)
        assert (r, st, got) == (0, -E["E_RANGE"], wb), (kind, toff)
        assert _ranges_raw(t, [((1 << 64) - 5, 10)] + ent) == (0, -E["E_RANGE"], [0x5A5A5A5A] + want)
        ixb = _dev(np.array([(0, o, ln) for o, ln in bad], np.uint64).tobytes())
        assert _code(D.crc32_ranges, t, ixb, len(bad)) == -E["E_RANGE"]
        # a status that is already there stays (compare-and-swap against 0)
        assert _ranges_raw(t, bad, st_init=-E["E_SZ"])[:2] == (0, -E["E_SZ"])
    assert D.lib().dmx_crc32_ranges_async(ctypes.c_void_p(base.data_ptr()), 10, None, 1, None, None, None) == -E["E_INVAL"]
    assert D.lib().dmx_crc32_ranges_async(ctypes.c_void_p(base.data_ptr()), 10, None, 0, None, None, None) == 0


# ---- corrupted files ----

def test_corrupted_stored_member_is_crc():
    n = HTS + 500
    data = _text(n, 38)
    z, lay = bgzf_file(data, hts_sizes(n), 0)
    assert z[18] & 6 == 0   # stored
    bad = bytearray(z)
    bad[18 + 5 + 40000] ^= 0x10   # a data byte past 32 768 bytes of the stored block: valid memory, a wrong byte
    bad = bytes(bad)
    assert _code(D.inflate_bgzf_gpu, bad) == -E["E_CRC"]
    assert _code(D.decompress_bgzf, bad) == -E["E_CRC"]
    idx, crcs, total = D.bgzf_index(bad, 65536)
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    assert _members(bad, idx, crcs, out.data_ptr(), total) == (0, -E["E_CRC"], total)
    assert _members(bad, idx, None, out.data_ptr(), total) == (0, 0, total)
    got = D.inflate_bgzf_gpu(bad, verify=False).cpu().numpy().tobytes()
    assert got != data and len(got) == n and got[:40000] == data[:40000]
    assert D.decompress_bgzf(bad, verify=False) == got


def test_broken_huffman_table_is_a_decode_status():
    """bit 17 of a dynamic block is the first bit of the first code length of the code length
    code; a code length code with one length changed is no longer complete (its Kraft sum moved),
    so the decode fails with -E_HUFAMB before any output, and that status stays: not -E_CRC"""
    n = HTS + 500
    data = _text(n, 39)
    z, lay = bgzf_file(data, hts_sizes(n), 6)
    assert z[18] & 6 == 4   # BTYPE 10: dynamic
    bad = bytearray(z)
    bad[18 + 2] ^= 0x02
    bad = bytes(bad)
    with pytest.raises(zlib.error):
        zlib.decompress(bad[18:lay[0][1] - 8], wbits=-15)
    assert _code(D.inflate_bgzf_gpu, bad) == -E["E_HUFAMB"]
    assert _code(D.decompress_bgzf, bad) == -E["E_HUFAMB"]
    idx, crcs, total = D.bgzf_index(bad, 65536)
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    r, st, _ = _members(bad, idx, crcs, out.data_ptr(), total)
    assert (r, st) == (0, -E["E_HUFAMB"])


# ---- limits, and what has not changed ----

def test_limits_and_unchanged_behaviour():
    sizes = [32769, 100]
    data = _text(sum(sizes), 40)
    z, _ = bgzf_file(data, sizes, 6)
    idx, crcs, total = D.bgzf_index(z, 65536)
    out = torch.empty(70000, dtype=torch.uint8, device="cuda")
    assert _members(z, idx, crcs, out.data_ptr(), total) == (0, 0, total)
    # an entry of 65 537 bytes is out of range, whatever the capacity
    big = idx.copy()
    big.view(np.uint32).reshape(-1, 6)[0, 4] = 65537
    r, st, _ = _members(z, big, None, out.data_ptr(), 70000)
    assert (r, st) == (0, -E["E_RANGE"])
    r, st, _ = _members(z, big, crcs, out.data_ptr(), 70000)   # and the CRC pass leaves that status
    assert (r, st) == (0, -E["E_RANGE"])
    # an entry that ends behind the capacity
    r, st, _ = _members(z, idx, crcs, out.data_ptr(), total - 1)
    assert (r, st) == (0, -E["E_RANGE"])
    # dmx_inflate_async keeps its bound: an entry of 32 769 bytes is -E_RANGE there
    dec, st = D.inflate_gpu(_dev(z), total, _dev(idx.tobytes()), 2)
    assert st == -E["E_RANGE"]
    # the project's own BGZF output decodes through the new path to the bytes of the old one
    own = _text(3 * 32768 + 17, 41)
    zo = D.compress(own, bgzf=True)
    io, co, to = D.bgzf_index(zo)
    assert entries(io) == entries(D.bgzf_index(zo, 65536)[0]) and to == len(own) and co.size == 4
    old, st = D.inflate_gpu(_dev(zo), to, _dev(io.tobytes()), 4)
    assert st == 0 and old.cpu().numpy().tobytes() == own
    assert D.inflate_bgzf_gpu(zo).cpu().numpy().tobytes() == own
    assert D.decompress_bgzf(zo) == own
    assert D.inflate_bgzf_gpu(b"").numel() == 0 and D.inflate_bgzf_gpu(bgzf_file(b"", [], 6)[0]).numel() == 0
    L = D.lib()
    assert L.dmx_inflate_members_async(None, 0, None, 0, None, 0, None, None, None) == -E["E_INVAL"]


# ---- graph capture ----

def test_members_async_in_a_graph():
    """dmx_inflate_members_async with CRCs captured once on a side stream and replayed twice: no
    hidden synchronisation, no allocation outside the stream-ordered pool"""
    sizes = [HTS, 0, 1, 40000]
    data = _text(sum(sizes), 42)
    z, _ = bgzf_file(data, sizes, 6)
    idx, crcs, total = D.bgzf_index(z, 65536)
    zt, ix, want = _dev(z), _dev(idx.tobytes()), _dev(crcs.tobytes())
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    st = torch.zeros(16, dtype=torch.uint8, device="cuda")
    L = D.lib()

    def enqueue():
        return L.dmx_inflate_members_async(ctypes.c_void_p(zt.data_ptr()), zt.numel(), ctypes.c_void_p(ix.data_ptr()),
                                           crcs.size, ctypes.c_void_p(out.data_ptr()), total,
                                           ctypes.c_void_p(want.data_ptr()), ctypes.c_void_p(st.data_ptr()),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the pool and the kernels exist before the capture
        assert enqueue() == 0
    side.synchronize()
    assert out.cpu().numpy().tobytes() == data
    g = torch.cuda.CUDAGraph()
    r = None
    try:
        with torch.cuda.graph(g, stream=side):
            r = enqueue()
    except RuntimeError as e:
        pytest.skip(f"the runtime refuses this capture (the pool allocation inside it): {e}")
    if r == -E["E_MALLOC"]:
        pytest.skip("the runtime refuses the pool allocation inside a stream capture (-E_MALLOC)")
    assert r == 0
    for k in range(2):
        out.zero_()
        st.fill_(0xEE)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        h = st.cpu().numpy()
        assert int(h[:4].view(np.int32)[0]) == 0 and int(h[8:16].view(np.uint64)[0]) == total, k
        assert out.cpu().numpy().tobytes() == data, k
    want[0] ^= 1   # the graph reads the CRCs where they are: a replay sees the wrong one
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert int(st.cpu().numpy()[:4].view(np.int32)[0]) == -E["E_CRC"]
