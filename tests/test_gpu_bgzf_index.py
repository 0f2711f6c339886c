"""The BGZF index built on the MI355X (dmx_bgzf_index_async, bgzf_index_gpu) and the device-to-device
decode on top of it (dmx_bgzf_decode_device, inflate_bgzf_tensor).  The host walk dmx_bgzf_index_max
is the specification: for the same bytes the device gives its status, count, total, entries and CRC
words -- compared over the whole output arrays, so also what an erring walk wrote before it stopped
-- on sound files, on truncated and corrupt ones and on files full of bytes that look like members.
One set of device buffers serves every case."""
import ctypes
import functools
import struct
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
from bgzf_read_inputs import EOF_MEMBER, HDR16, HTS, TOP, bgzf_file, hts_sizes, member

pytestmark = pytest.mark.gpu

E = D.E
SZ, RANGE, CRC = -E["E_SZ"], -E["E_RANGE"], -E["E_CRC"]
GUARD = 0xEE
ZCAP = 1 << 20      # the file buffer
CAPMAX = 4096       # entries the result buffer holds
FIVE = [1, 32768, 32769, HTS, TOP]


@functools.lru_cache(maxsize=None)
def _text(n: int, seed: int = 51) -> bytes:
    return D.gen_text(max(n, 1), seed).tobytes()[:n]


def _tile() -> int:
    t = ctypes.c_uint32(0)
    D.lib().dmx_bgzf_index_geometry(ctypes.byref(t))
    return t.value


class Bufs:
    """the device buffers of every case: the file (with room to shift it), one result block
    [record 32 B | entries | CRC words], the work buffer"""

    def __init__(self):
        L = D.lib()
        self.z = torch.zeros(ZCAP + 64, dtype=torch.uint8, device="cuda")
        self.res = torch.zeros(32 + CAPMAX * 28, dtype=torch.uint8, device="cuda")
        self.max_cand = ZCAP // 26 + 8
        self.work_bytes = int(L.dmx_bgzf_index_work(ZCAP, self.max_cand))
        self.work = torch.zeros(self.work_bytes, dtype=torch.uint8, device="cuda")
        assert self.z.data_ptr() % 256 == 0 and self.res.data_ptr() % 256 == 0 and self.work.data_ptr() % 256 == 0


@functools.lru_cache(maxsize=None)
def _bufs() -> Bufs:
    return Bufs()


def _upload(z: bytes, head: int = 0):
    B = _bufs()
    assert len(z) <= ZCAP and 0 <= head < 64
    if z:
        B.z[head:head + len(z)].copy_(torch.from_numpy(np.frombuffer(z, np.uint8).copy()))


def _enqueue(n: int, max_isize: int, cap: int, head: int = 0, work_bytes=None, stream=None) -> int:
    B = _bufs()
    assert cap <= CAPMAX
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    p = B.res.data_ptr()
    return D.lib().dmx_bgzf_index_async(ctypes.c_void_p(B.z.data_ptr() + head), n, max_isize, ctypes.c_void_p(p + 32),
                                        ctypes.c_void_p(p + 32 + cap * 24), cap, ctypes.c_void_p(B.work.data_ptr()),
                                        B.work_bytes if work_bytes is None else work_bytes, ctypes.c_void_p(p),
                                        ctypes.c_void_p(s))


def _result(cap: int):
    """(status, nblk, total, ncand, reserved, entry bytes, CRC bytes) of the result block"""
    h = _bufs().res[:32 + cap * 28].cpu().numpy()
    return (int(h[:4].view(np.int32)[0]), int(h[4:8].view(np.uint32)[0]), int(h[8:16].view(np.uint64)[0]),
            int(h[16:20].view(np.uint32)[0]), int(h[20:24].view(np.uint32)[0]), h[32:32 + cap * 24].tobytes(),
            h[32 + cap * 24:32 + cap * 28].tobytes())


def _device(n: int, max_isize: int = 65536, cap: int = 8, head: int = 0, work_bytes=None):
    """the device index of the n bytes uploaded at `head`, into arrays filled with GUARD"""
    _bufs().res[:32 + cap * 28].fill_(GUARD)
    assert _enqueue(n, max_isize, cap, head, work_bytes) == 0
    return _result(cap)


def _host(z: bytes, max_isize: int = 65536, cap: int = 8):
    """(status, nblk, total, entry bytes, CRC bytes) of dmx_bgzf_index_max, arrays filled with GUARD"""
    idx = np.full(cap * 24 + 8, GUARD, np.uint8)
    crc = np.full(cap * 4 + 4, GUARD, np.uint8)
    buf = (ctypes.c_uint8 * max(len(z), 1)).from_buffer_copy(z or b"\0")
    nb, tot = ctypes.c_uint32(0), ctypes.c_uint64(0)
    r = D.lib().dmx_bgzf_index_max(buf, len(z), max_isize, ctypes.c_void_p(idx.ctypes.data), ctypes.c_void_p(crc.ctypes.data),
                                   cap, ctypes.byref(nb), ctypes.byref(tot))
    return r, nb.value, tot.value, idx[:cap * 24].tobytes(), crc[:cap * 4].tobytes()


def _same(z: bytes, max_isize: int = 65536, cap: int = 8, head: int = 0, n=None, what=""):
    """the device index of z[:n] (z already uploaded at `head` where n is given) equals the host walk"""
    if n is None:
        _upload(z, head)
        n = len(z)
    hs, hn, ht, hi, hc = _host(z[:n], max_isize, cap)
    ds, dn, dt, dc, dr, di, dcrc = _device(n, max_isize, cap, head)
    assert (ds, dn, dt, dr) == (hs, hn, ht, 0), (what, n, max_isize, cap, head, (ds, dn, dt), (hs, hn, ht))
    assert di == hi, (what, n, "entries")
    assert dcrc == hc, (what, n, "CRC words")
    return hs, hn, ht, dc


@functools.lru_cache(maxsize=None)
def _long_file():
    """3 000 members of one byte, an empty member after every seventh: a chain longer than a wave, a
    workgroup and 2^11, over at least three scan tiles (stored members in front where the tile is
    larger than that)"""
    sizes = []
    for k in range(3000):
        sizes.append(1)
        if k % 7 == 6:
            sizes.append(0)
    data = _text(3000, 52)
    z, _ = bgzf_file(data, sizes, 6)
    pad = b""
    while len(pad) + len(z) < 3 * _tile():
        pad += member(_text(HTS, 53), 0)
    return pad + z, (_text(HTS, 53) * (len(pad) // len(member(_text(HTS, 53), 0)))) + data


# ---- 1. sound files ----

def _sound_files():
    n3 = 3 * HTS + 17
    return [("five", bgzf_file(_text(sum(FIVE), 54), FIVE, 1)[0]),
            ("hts", bgzf_file(_text(n3, 55), hts_sizes(n3), 6)[0]),
            ("mixed", bgzf_file(_text(1234 + HTS + 3486, 56), [1234, 0, HTS, 3486], 6)[0]),
            ("empty", b""),
            ("eof", EOF_MEMBER),
            ("eof2", EOF_MEMBER * 2),
            ("own", D.compress(D.gen_text(100000), sw=4096, bgzf=True)),
            ("long", _long_file()[0])]


def test_sound_files():
    tile = _tile()
    for name, z in _sound_files():
        status, nblk, total, ncand = _same(z, 65536, CAPMAX, what=name)
        assert status == 0, name
        assert ncand >= nblk
        if name == "long":
            assert nblk >= 3000 and len(z) >= 3 * tile and ncand > 2048
        if name == "own":
            assert nblk == 25 and total == 100000
        # the Python entry point gives the same tensors
        zt = _bufs().z[:len(z)]
        ix, crcs, nb, tot = D.bgzf_index_gpu(zt)
        hidx, hcrc, htot = D.bgzf_index(z, 65536)
        assert (nb, tot) == (hcrc.size, htot) and ix.cpu().numpy().tobytes() == hidx.tobytes(), name
        assert crcs.cpu().numpy().view(np.uint32).tolist() == hcrc.tolist(), name


# ---- 2. cap and the bound on a member ----

def test_cap_and_bounds():
    z = bgzf_file(_text(sum(FIVE), 54), FIVE, 1)[0]
    _upload(z)
    for cap in (0, 2, 5, 6):
        status, nblk, total, _ = _same(z, 65536, cap, n=len(z), what=f"cap {cap}")
        assert status == (SZ if cap < 5 else 0) and nblk == 5 and total == sum(FIVE)
    for bound in (1, 32768, 65279, 65280, 65535):
        assert _same(z, bound, 8, n=len(z), what=f"bound {bound}")[0] == RANGE
    n3 = 3 * HTS + 17
    z = bgzf_file(_text(n3, 55), hts_sizes(n3), 6)[0]
    _upload(z)
    for bound, want in ((65279, RANGE), (65280, 0), (65536, 0)):
        assert _same(z, bound, 8, n=len(z), what=f"hts bound {bound}")[0] == want
    with pytest.raises(D.DeflateError) as e:
        D.bgzf_index_gpu(_bufs().z[:len(z)], max_member=65279)
    assert e.value.code == RANGE
    with pytest.raises(D.DeflateError) as e:
        D.bgzf_index_gpu(_bufs().z[:len(z)], cap=2)
    assert e.value.code == SZ


# ---- 3. truncations ----

@pytest.mark.parametrize("level", [6, 0])
def test_every_truncation(level):
    z = bgzf_file(_text(400, 57), [300, 100], level)[0]
    _upload(z + bytes([0x1F, 0x8B, 8, 4]) * 8)   # what lies behind the cut is never looked at
    seen = set()
    for t in range(len(z) + 1):
        seen.add(_same(z, 65536, 4, n=t, what=f"cut {t}")[0])
    assert seen == {0, -E["E_LEN"]}   # a cut at a member's end leaves a sound file


# ---- 4. bit flips ----

def test_every_header_and_trailer_bit_flip():
    z, lay = bgzf_file(_text(900, 58), [500, 0, 400], 6, eof=False)
    assert len(lay) == 3
    seen = set()
    for p, size, _, _ in lay:
        for q in list(range(p, p + 18)) + list(range(p + size - 8, p + size)):
            for bit in range(8):
                f = bytearray(z)
                f[q] ^= 1 << bit
                seen.add(_same(bytes(f), 65536, 4, what=f"flip {q}.{bit}")[0])
    assert {0, -E["E_ZHEAD"], -E["E_LEN"], RANGE} <= seen


# ---- 5. look-alikes ----

def _stored(data: bytes, crc=None, isize=None) -> bytes:
    """a member of one stored block around data, by hand: its size is len(data) + 31"""
    d = b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data
    size = 18 + len(d) + 8
    assert len(data) <= 65535 and size <= 65536
    return HDR16 + struct.pack("<H", size - 1) + d + struct.pack("<II", zlib.crc32(data) if crc is None else crc,
                                                                 len(data) if isize is None else isize)


def _with_fake(total: int, pos: int, seed: int = 59) -> bytes:
    """a stored member of `total` bytes whose data spells, at offset pos of the member, a member
    header whose BSIZE ends where this member ends: a false chain that merges into the true one"""
    n = total - 31
    fake = HDR16 + struct.pack("<H", total - pos - 1)
    at = pos - 23
    assert 0 <= at and at + 18 + 8 <= n
    data = bytearray(_text(n, seed))
    data[at:at + 18] = fake
    m = _stored(bytes(data))
    assert len(m) == total and m[pos:pos + 18] == fake
    return m


def test_bgzf_file_inside_a_stored_member():
    inner, _ = bgzf_file(_text(3000, 41), [1000, 1500, 500], 6)
    z = _stored(inner) + member(_text(700, 60), 6) + EOF_MEMBER
    status, nblk, total, ncand = _same(z, what="nested")
    assert (status, nblk, total) == (0, 2, len(inner) + 700) and ncand == 3 + 4   # the inner members parse too


def test_false_chain_merges_into_the_true_one():
    z = _with_fake(5000, 1000) + member(_text(700, 60), 6) + member(b"", 6) + member(_text(9, 61), 6) + EOF_MEMBER
    status, nblk, total, ncand = _same(z, what="merge")
    assert (status, nblk, total, ncand) == (0, 3, 4969 + 709, 6)
    # the same with fakes behind a few true members
    z2 = member(_text(50, 62), 6) * 3 + _with_fake(4000, 100) + _with_fake(3000, 2000) + EOF_MEMBER
    assert _same(z2, what="merge 2")[:2] == (0, 5)


def test_fake_header_just_before_a_member_start():
    fake = HDR16 + struct.pack("<H", 99)
    base = _stored(_text(64, 64))
    tail = member(_text(300, 63), 6) + EOF_MEMBER
    for k in range(1, 18):
        m = bytearray(base)
        m[len(m) - k:] = fake[:k]     # the header's first k bytes end the member, trailer included; the next member follows
        _same(bytes(m) + tail, what=f"before {k}")
        if k > 8:                      # the same with the trailer left as it was: the header's start in the data alone
            m = bytearray(base)
            m[len(m) - k:len(m) - 8] = fake[:k - 8]
            assert _same(bytes(m) + tail, what=f"before {k}, trailer kept")[:2] == (0, 2)


def test_members_and_fakes_around_a_tile_edge():
    tile = _tile()
    assert tile - 18 >= 64 and tile + 1 + 31 <= 65536
    tail = member(_text(300, 63), 6) + EOF_MEMBER
    for off in range(tile - 18, tile + 2):
        z = _stored(_text(off - 31, 65)) + tail            # a true member starts at `off`
        assert z[off:off + 4] == HDR16[:4]
        status, nblk, _, _ = _same(z, what=f"true at {off}")
        assert (status, nblk) == (0, 2)
        z = _with_fake(off + 200, off, 66) + tail           # a fake header at `off`
        status, nblk, _, ncand = _same(z, what=f"fake at {off}")
        assert (status, nblk, ncand) == (0, 2, 4)


# ---- 6. header variants ----

def _variant(block: bytes, before: bytes = b"", after: bytes = b"", name: bytes = b"", comment: bytes = b"",
             hcrc: bool = False) -> bytes:
    c = zlib.compressobj(6, wbits=-15)
    d = c.compress(block) + c.flush()
    flg = 4 | (8 if name else 0) | (16 if comment else 0) | (2 if hcrc else 0)
    extra = before + b"BC\x02\x00" + b"\0\0" + after
    h = bytes([0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", len(extra)) + extra + name + comment
    h += b"\x12\x34" if hcrc else b""
    size = len(h) + len(d) + 8
    at = 12 + len(before) + 4
    h = h[:at] + struct.pack("<H", size - 1) + h[at + 2:]
    return h + d + struct.pack("<II", zlib.crc32(block), len(block))


def test_header_variants():
    sub = b"XY\x03\x00abc"
    ms = [_variant(_text(100, 67), before=sub), _variant(_text(200, 68), after=sub + b"ZZ\x00\x00"),
          _variant(_text(300, 69), before=sub, after=sub, name=b"reads.bam\0"),
          _variant(_text(50, 70), name=b"n\0", comment=b"made by hand\0", hcrc=True), member(_text(10, 71), 6)]
    z = b"".join(ms) + EOF_MEMBER
    status, nblk, total, _ = _same(z, what="variants")
    assert (status, nblk, total) == (0, 5, 660)
    hidx, _, _ = D.bgzf_index(z, 65536)
    bodies = [int(b) // 8 for b in hidx.view(np.uint64).reshape(-1, 3)[:, 0]]
    assert bodies[0] == 18 + 7 and bodies[2] - len(ms[0]) - len(ms[1]) == 18 + 14 + 10   # the DEFLATE data behind each header
    assert D.inflate_bgzf_tensor(_bufs().z[:len(z)]).cpu().numpy().tobytes() == b"".join(_text(n, s) for n, s in
                                                                                      ((100, 67), (200, 68), (300, 69), (50, 70), (10, 71)))
    # a subfield that runs past XLEN, an unterminated name: the walk's status
    bad = bytearray(ms[0])
    bad[14:16] = struct.pack("<H", 200)
    _same(bytes(bad) + EOF_MEMBER, what="subfield past XLEN")
    bad = bytearray(_variant(_text(40, 72), name=b"x\0"))
    bad[3] |= 16
    for k in range(18, len(bad)):
        bad[k] = bad[k] or 1
    _same(bytes(bad) + EOF_MEMBER, what="comment without end")


# ---- 7. alignment ----

@pytest.mark.parametrize("head", [1, 15])
def test_unaligned_file(head):
    _bufs().z.fill_(0x1F)   # the bytes around the file are not zeros
    for name, z in (("five", bgzf_file(_text(sum(FIVE), 54), FIVE, 1)[0]), ("long", _long_file()[0]),
                    ("merge", _with_fake(5000, 1000) + EOF_MEMBER), ("short", EOF_MEMBER[:11])):
        _same(z, 65536, CAPMAX, head=head, what=f"{name} at {head}")
    zt = _bufs().z[head:head + len(z)]
    assert zt.storage_offset() == head


# ---- 8. work buffer overflow ----

def test_work_overflow_and_retry():
    L = D.lib()
    z = bgzf_file(_text(300, 44), [1] * 300, 6)[0]
    _upload(z)
    small = int(L.dmx_bgzf_index_work(len(z), 4))
    status, nblk, total, ncand, _, _, _ = _device(len(z), 65536, 8, work_bytes=small)
    assert (status, nblk, total, ncand) == (SZ, 0, 0, 301)
    exact = int(L.dmx_bgzf_index_work(len(z), 301))
    hs, hn, ht, hi, hc = _host(z, 65536, 300)
    ds, dn, dt, dc, _, di, dcrc = _device(len(z), 65536, 300, work_bytes=exact)
    assert (ds, dn, dt, dc) == (hs, hn, ht, 301) == (0, 300, 300, 301) and di == hi and dcrc == hc


# ---- 9. decode ----

def test_decode_device_to_device():
    n3 = 3 * HTS + 17
    for data, z in ((_text(n3, 55), bgzf_file(_text(n3, 55), hts_sizes(n3), 6)[0]), (_long_file()[1], _long_file()[0])):
        _upload(z)
        zt = _bufs().z[:len(z)]
        assert D.inflate_bgzf_tensor(zt).cpu().numpy().tobytes() == data
        assert D.inflate_bgzf_tensor(zt, verify=False).cpu().numpy().tobytes() == data
    assert D.inflate_bgzf_tensor(torch.empty(0, dtype=torch.uint8, device="cuda")).numel() == 0
    _upload(EOF_MEMBER * 2)
    assert D.inflate_bgzf_tensor(_bufs().z[:56]).numel() == 0


def test_decode_encoder_output_in_place():
    data = D.gen_text(150000, 73)
    t = torch.from_numpy(data.copy()).cuda()
    enc = D.Encoder(0, len(data))
    try:
        zt, r = enc.compress_tensor(t, opts=D.Opts(32768, 0, D.DMX_BGZF, 0))
        assert r.status == 0
        out = D.inflate_bgzf_tensor(zt)      # the encoder's tensor, as it lies in HBM
        assert torch.equal(out, t)
    finally:
        enc.close()


def test_decode_crc_and_capacity():
    L = D.lib()
    data = _text(2 * HTS + 100, 74)
    z, lay = bgzf_file(data, hts_sizes(len(data)), 6)
    f = bytearray(z)
    f[lay[1][0] + lay[1][1] - 8] ^= 0x10    # the second member's stored CRC-32
    _upload(bytes(f))
    zt = _bufs().z[:len(z)]
    with pytest.raises(D.DeflateError) as e:
        D.inflate_bgzf_tensor(zt, verify=True)
    assert e.value.code == CRC
    assert D.inflate_bgzf_tensor(zt, verify=False).cpu().numpy().tobytes() == data
    _upload(z)
    out = torch.full((len(data),), 0x5A, dtype=torch.uint8, device="cuda")
    olen = ctypes.c_uint64(0)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = L.dmx_bgzf_decode_device(ctypes.c_void_p(zt.data_ptr()), len(z), ctypes.c_void_p(out.data_ptr()), len(data) - 1,
                                 ctypes.byref(olen), 1, s)
    torch.cuda.synchronize()
    assert r == SZ and olen.value == len(data) and bool((out == 0x5A).all())
    r = L.dmx_bgzf_decode_device(ctypes.c_void_p(zt.data_ptr()), len(z), ctypes.c_void_p(out.data_ptr()), len(data),
                                 ctypes.byref(olen), 1, s)
    torch.cuda.synchronize()
    assert r == 0 and olen.value == len(data) and out.cpu().numpy().tobytes() == data
    # a file that does not index: the walk's status, no length
    r = L.dmx_bgzf_decode_device(ctypes.c_void_p(zt.data_ptr()), len(z) - 5, ctypes.c_void_p(out.data_ptr()), len(data),
                                 ctypes.byref(olen), 1, s)
    assert r == -E["E_LEN"] and olen.value == 0


# ---- 10. graph capture ----

def test_index_in_a_graph():
    """dmx_bgzf_index_async captured once on a side stream -- kernels only, one after the other --
    and replayed on two files of one length that lie in the same buffers"""
    za = _stored(_text(300, 75)) + _stored(_text(100, 76)) + EOF_MEMBER
    zb = _stored(_text(100, 77)) + _stored(b"") + _stored(_text(269, 78)) + EOF_MEMBER
    assert len(za) == len(zb) == 490
    n, cap = len(za), 8
    side = torch.cuda.Stream()
    _upload(za)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the kernels are loaded before the capture
        assert _enqueue(n, 65536, cap) == 0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r = _enqueue(n, 65536, cap)
    assert r == 0
    blocks = []
    for z in (za, zb, zb, za):
        _upload(z)
        _bufs().res[:32 + cap * 28].fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ds, dn, dt, _, dr, di, dcrc = _result(cap)
        hs, hn, ht, hi, hc = _host(z, 65536, cap)
        assert (ds, dn, dt, dr) == (hs, hn, ht, 0) and di == hi and dcrc == hc
        blocks.append(_bufs().res[:32 + cap * 28].cpu().numpy().tobytes())
    assert blocks[1] == blocks[2] and blocks[0] == blocks[3] and blocks[0] != blocks[1]
