"""BGZF container (DMX_F_BGZF) on the MI355X: the per-block CRC-32 kernel against zlib.crc32 at
every block size around the lane slice and the span, with unaligned bases; the BGZF encode byte
for byte (per block: header with BSIZE + the oracle's DEFLATE data of the block alone + CRC-32
/ ISIZE, then the end-of-file member) under every launch shape; the output bound; shards; the
round trip through the host index and the GPU inflate with the per-member CRC check; a foreign
BGZF file; the file path; no flag state left behind."""
import ctypes
import functools
import gzip
import os
import struct
import threading
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
from deflate_compression_amd import shard
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HDR16 = bytes([0x1F, 0x8B, 0x08, 0x04, 0, 0, 0, 0, 0, 0xFF, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00])
EOF_MEMBER = HDR16 + bytes([0x1B, 0x00, 0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0])
HDR10 = bytes([0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0, 0xFF])
BLK = 32768
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def enc():
    e = D.Encoder(0, 2 << 20)
    yield e
    e.close()


# ---- the per-block CRC-32 kernel ----

def _crc_blocks_guarded(e, t, n, sw):
    """dmx_crc32_blocks_async into a buffer with a guard word behind the last block's"""
    nb = (n + sw - 1) // sw
    w = torch.full((nb + 1,), GUARD, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if not s:
        torch.cuda.synchronize()
    r = e._L.dmx_crc32_blocks_async(e._ctx, ctypes.c_void_p(t.data_ptr() if n else 0), n, sw,
                                    ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(s))
    assert r == 0
    torch.cuda.synchronize()
    h = w.cpu().numpy().view(np.uint32)
    assert h[nb] == GUARD, "the word behind d_crc was written"
    return h[:nb]


@pytest.mark.parametrize("kind", ["random", "zeros", "ff"])
def test_crc32_blocks_vs_zlib(enc, kind):
    S, L = D.crc32_geometry()
    sws = [1, 15, 16, 17, L - 1, L, L + 1, 4097, 32767, 32768]
    top = 3 * 32768 + 5
    h = {"random": np.random.default_rng(41).integers(0, 256, top, dtype=np.uint8), "zeros": np.zeros(top, np.uint8),
         "ff": np.full(top, 0xFF, np.uint8)}[kind]
    hb = h.tobytes()
    base = torch.empty(top + 256 + 16, dtype=torch.uint8, device="cuda")
    a0 = (-base.data_ptr()) % 256   # a 256-byte aligned start inside the tensor
    for off in (0, 1, 3, 15):
        t = base[a0 + off:a0 + off + top]
        assert t.data_ptr() % 256 == off
        t.copy_(torch.from_numpy(h))
        for sw in sws:
            for n in (1, sw - 1, sw, sw + 1, 3 * sw + 5):
                got = _crc_blocks_guarded(enc, t, n, sw)
                want = [zlib.crc32(hb[o:min(o + sw, n)]) for o in range(0, n, sw)]
                assert got.tolist() == want, (kind, off, sw, n)
    # the tensor wrapper, and the argument checks
    assert enc.crc32_blocks(t[:70000], 32768).cpu().numpy().view(np.uint32).tolist() == \
        [zlib.crc32(hb[o:min(o + 32768, 70000)]) for o in range(0, 70000, 32768)]   # (t: the last base, offset 15)
    w = torch.zeros(4, dtype=torch.int32, device="cuda")
    for sw in (-1, 32769):
        assert enc._L.dmx_crc32_blocks_async(enc._ctx, ctypes.c_void_p(base.data_ptr()), 10, sw,
                                             ctypes.c_void_p(w.data_ptr()), None) == -D.E["E_RANGE"]


# ---- the encode ----

def _mixed(nblk, tail=0):
    """random / text alternating per block: stored blocks at non-zero offsets"""
    parts = []
    for b in range(nblk):
        parts.append(D.gen_random(BLK, 100 + b).tobytes() if b % 2 == 0 else D.gen_text(BLK, 200 + b).tobytes())
    if tail:
        parts.append(D.gen_text(tail, 77).tobytes())
    return b"".join(parts)


SIZES = [0, 1, 2, 32767, 32768, 32769, 65541, 5 * BLK + 1]


@functools.lru_cache(maxsize=None)
def _input(kind: str, n: int) -> bytes:
    if kind == "text":
        return D.gen_text(max(n, 1), 5).tobytes()[:n]
    if kind == "random":
        return D.gen_random(max(n, 1), 6).tobytes()[:n]
    if kind == "zeros":
        return bytes(n)
    return _mixed((n + BLK - 1) // BLK)[:n]


FAST = D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK
FAST_KW = dict(max_chain=7, lazy=True, deep=True, store_check=True)


@functools.lru_cache(maxsize=None)
def _member(block: bytes, sw: int, fast) -> bytes:
    """block as a BGZF member: the oracle's zlib stream of the block alone without its 2 + 4
    bytes of framing, behind the 18-byte header, before CRC-32 and ISIZE (fast: False = the
    plain options, True = max_chain 7 with LAZY, DEEP and STORE_CHECK, "check" = STORE_CHECK alone)"""
    kw = dict(store_check=True) if fast == "check" else FAST_KW if fast else {}
    d = O.compress(block, sw=sw, **kw)[2:-4]
    return HDR16 + struct.pack("<H", 18 + len(d) + 8 - 1) + d + struct.pack("<II", zlib.crc32(block), len(block))


def _want(data: bytes, sw: int = BLK, fast=False, final: bool = True) -> bytes:
    return b"".join(_member(data[o:o + sw], sw, fast) for o in range(0, len(data), sw)) + (EOF_MEMBER if final else b"")


def _check_result(r, z: bytes, rz):
    """dmx_result under DMX_BGZF against the bytes and the zlib encode's result rz"""
    assert r.out_len == len(z) and r.adler == 0 and r.end_bits == 8 * (len(z) - 28)
    assert (r.nblocks, r.nstored, r.nfixed, r.ndynamic, r.ntokens) == \
        (rz.nblocks, rz.nstored, rz.nfixed, rz.ndynamic, rz.ntokens)


@pytest.mark.parametrize("kind", ["text", "random", "zeros", "mixed"])
def test_bgzf_encode_byte_identical(enc, kind):
    for n in SIZES:
        data = _input(kind, n)
        nblk = (n + BLK - 1) // BLK
        for fast in (False, True):
            kw = dict(max_chain=7, flags=D.DMX_BGZF | FAST) if fast else dict(flags=D.DMX_BGZF)
            z, r = enc.compress_bytes(data, **kw)
            assert z == _want(data, fast=fast), (kind, n, fast)
            assert gzip.decompress(z) == data, (kind, n, fast)
            got = [a.tolist() for a in enc.blocks(nblk)] if nblk else []
            kz = dict(kw, flags=(kw["flags"] & ~D.DMX_BGZF) | D.DMX_ZLIB)
            _, rz = enc.compress_bytes(data, **kz)
            _check_result(r, z, rz)
            assert got == ([a.tolist() for a in enc.blocks(nblk)] if nblk else []), (kind, n, fast)


def test_bgzf_small_window(enc):
    sw, n = 4097, 3 * 4097 + 17
    data = _input("mixed", BLK)[BLK - 6000:] + _input("text", n)   # noise first, then text
    data = data[:n]
    for fast in (False, True):
        kw = dict(max_chain=7, flags=D.DMX_BGZF | FAST) if fast else dict(flags=D.DMX_BGZF)
        z, r = enc.compress_bytes(data, sw=sw, **kw)
        assert z == _want(data, sw=sw, fast=fast), fast
        assert gzip.decompress(z) == data and r.nblocks == 4 and r.out_len == len(z) and r.adler == 0


@pytest.mark.parametrize("worklist", ["0", "list", "plain"])
@pytest.mark.parametrize("scan3", [0, 1])
def test_bgzf_under_hook_shapes(worklist, scan3):
    e = D.Encoder(0, 1 << 20)   # a context of its own: the module's keeps its hooks
    try:
        e.set_hook("worklist", worklist)
        e.set_hook("scan3", scan3)
        for n in (0, 1, 32769, 5 * BLK + 1):
            data = _input("mixed", n)
            z, _ = e.compress_bytes(data, max_chain=7, flags=D.DMX_BGZF | FAST)
            assert z == _want(data, fast=True), (worklist, scan3, n)
            z, _ = e.compress_bytes(data, flags=D.DMX_BGZF | D.DMX_F_STORE_CHECK)
            assert z == _want(data, fast="check"), (worklist, scan3, n)
        rnd = _input("random", 5 * BLK + 1)   # all stored: no speculative copy, no whole-copy prefix under the flag
        zer = _input("zeros", 5 * BLK + 1)    # uniform blocks: the dedupe copies whole members
        for _ in range(2):   # (the second encode runs with the first one's launch-shape hint)
            z, _ = e.compress_bytes(rnd, max_chain=7, flags=D.DMX_BGZF | FAST)
            assert z == _want(rnd, fast=True), (worklist, scan3)
        for dd in (None, 1):
            e.set_hook("dedupe", dd)
            for _ in range(2):
                z, _ = e.compress_bytes(zer, max_chain=7, flags=D.DMX_BGZF | FAST)
                assert z == _want(zer, fast=True), (worklist, scan3, dd)
    finally:
        e.set_hook("worklist", None)
        e.set_hook("scan3", 0)
        e.set_hook("dedupe", None)
        e.close()


def test_bgzf_capacity(enc):
    n = 3 * BLK
    data = _input("random", n)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    o = D.Opts(BLK, 0, D.DMX_BGZF, 0)
    cap = D.max_compressed(n, BLK, D.DMX_BGZF)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    enc.reserve(n, BLK)
    torch.cuda.synchronize()   # (the encodes below run on the context's own stream)
    enc.encode_async(t.data_ptr(), n, out.data_ptr(), cap, None, o)
    r = enc.result()
    z = out[:r.out_len].cpu().numpy().tobytes()
    assert r.out_len == 3 * (BLK + 31) + 28 and gzip.decompress(z) == data
    rounded = (r.out_len + 3) & ~3
    enc.encode_async(t.data_ptr(), n, out.data_ptr(), rounded, None, o)   # exactly enough
    assert enc.result().out_len == r.out_len
    enc.encode_async(t.data_ptr(), n, out.data_ptr(), rounded - 4, None, o)
    with pytest.raises(D.DeflateError) as ei:
        enc.result()
    assert ei.value.code == -D.E["E_SZ"]


def test_bgzf_without_final_and_shards(enc):
    n = 4 * BLK + 100
    data = _input("text", n)
    whole, _ = enc.compress_bytes(data, flags=D.DMX_BGZF)
    assert whole == _want(data)
    z, r = enc.compress_bytes(data, flags=D.DMX_F_BGZF)   # no end-of-file member, no flush
    assert z == whole[:-28] and r.out_len == len(z) and r.end_bits == 8 * len(z)
    # the stream framing flags are ignored under the flag
    z, _ = enc.compress_bytes(data, flags=D.DMX_F_BGZF | D.DMX_GZIP)
    assert z == whole
    z, r = enc.compress_bytes(b"", flags=D.DMX_F_BGZF)
    assert z == b"" and r.out_len == 0
    z, r = enc.compress_bytes(b"", flags=D.DMX_BGZF)
    assert z == EOF_MEMBER and r.end_bits == 0 and r.adler == 0
    cuts = [0, BLK, 3 * BLK, n]
    pieces = [enc.compress_bytes(data[cuts[k]:cuts[k + 1]], flags=shard.shard_flags_bgzf(k, 3))[0] for k in range(3)]
    assert b"".join(pieces) == whole


def test_bgzf_flag_conflicts_leave_no_state(enc):
    data = _input("mixed", 5 * BLK + 1)
    for bad in (D.DMX_F_DICT, D.DMX_F_SPLIT, D.DMX_F_DICT | D.DMX_F_SPLIT):
        with pytest.raises(D.DeflateError) as ei:
            enc.compress_bytes(data, flags=D.DMX_BGZF | bad)
        assert ei.value.code == -D.E["E_INVAL"]
    z, _ = enc.compress_bytes(data, max_chain=7, flags=D.DMX_BGZF | FAST)
    assert z == _want(data, fast=True)
    z, r = enc.compress_bytes(data, max_chain=7, flags=D.DMX_ZLIB | FAST)
    assert z == O.compress(data, **FAST_KW) and r.adler == zlib.adler32(data)
    z, r = enc.compress_bytes(data, flags=D.DMX_GZIP)
    assert z == HDR10 + O.compress(data)[2:-4] + struct.pack("<II", zlib.crc32(data), len(data))
    assert r.adler == zlib.crc32(data)


@pytest.mark.parametrize("n", [0, 1000, 3 * BLK + 17])
def test_compress_host_buffer_bgzf(n):
    """dmx_encode_host under DMX_F_BGZF (compress(bgzf=True)): sized by the BGZF bound."""
    data = _input("mixed", n)
    assert D.compress(data, bgzf=True) == _want(data)
    assert D.compress(data, flags=D.DMX_BGZF, max_chain=7, lazy=True, deep=True, store_check=True) == _want(data, fast=True)
    assert D.compress(data) == O.compress(data)   # and zlib on the same cached context after it


# ---- the reader ----

def test_bgzf_round_trip_on_the_gpu(enc):
    n = 4 * BLK + 12345
    data = _input("mixed", n)   # block 0 is noise: a stored member
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    out, r = enc.compress_tensor(t, opts=D.Opts(BLK, 0, D.DMX_BGZF, 0))
    ix, nb = enc.block_index()
    z = out.cpu().numpy().tobytes()
    idx, crcs, total = D.bgzf_index(z)
    assert total == n and nb == crcs.size == 5
    assert ix.cpu().numpy().tobytes() == idx.tobytes()
    assert crcs.tolist() == [zlib.crc32(data[o:o + BLK]) for o in range(0, n, BLK)]
    dec, st = D.inflate_gpu(out, n, torch.from_numpy(idx.copy()).cuda(), nb)
    assert st == 0 and dec.cpu().numpy().tobytes() == data
    assert D.inflate_bgzf_gpu(z, encoder=enc).cpu().numpy().tobytes() == data
    assert D.inflate_bgzf_gpu(z).cpu().numpy().tobytes() == data
    # one flipped bit in the stored member's data: valid memory, a wrong byte, -E_CRC
    assert r.nstored >= 1 and z[18] == 0x01   # BFINAL = 1, BTYPE = 00
    bad = bytearray(z)
    bad[18 + 5 + 100] ^= 0x10
    with pytest.raises(D.DeflateError) as ei:
        D.inflate_bgzf_gpu(bytes(bad), encoder=enc)
    assert ei.value.code == -D.E["E_CRC"]
    assert D.inflate_bgzf_gpu(bytes(bad), verify=False, encoder=enc).cpu().numpy().tobytes() != data


def _foreign(data: bytes, level: int, msize: int = 20000) -> bytes:
    """a BGZF file as another writer makes it: zlib raw deflate per member, a full flush in
    the middle of every member (several DEFLATE blocks, an empty stored one among them)"""
    out = []
    for o in range(0, len(data), msize):
        blk = data[o:o + msize]
        c = zlib.compressobj(level, wbits=-15)
        d = c.compress(blk[:len(blk) // 2]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(blk[len(blk) // 2:]) + c.flush()
        out.append(HDR16 + struct.pack("<H", 18 + len(d) + 8 - 1) + d + struct.pack("<II", zlib.crc32(blk), len(blk)))
    return b"".join(out) + EOF_MEMBER


@pytest.mark.parametrize("level", [0, 1, 9])
def test_foreign_bgzf_file(enc, level):
    data = _input("text", 50000)
    z = _foreign(data, level)
    assert gzip.decompress(z) == data
    assert D.inflate_bgzf_gpu(z, encoder=enc).cpu().numpy().tobytes() == data
    with pytest.raises(D.DeflateError) as ei:
        D.bgzf_index(_foreign(data, level, 40000))
    assert ei.value.code == -D.E["E_RANGE"]


# ---- the file path ----

def _fd(tmp_path, data: bytes, env: dict, pipe_in: bool = False, stats: bool = False):
    fi, fo, fs = tmp_path / "in", tmp_path / "out", tmp_path / "stats"
    fi.write_bytes(data)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with open(fo, "wb") as b, open(fs, "wb") as s:
            sfd = s.fileno() if stats else -1
            if pipe_in:
                r, w = os.pipe()
                feeder = threading.Thread(target=lambda: (os.write(w, data), os.close(w)))
                feeder.start()
                try:
                    rc = D.deflate_compress(r, b.fileno(), sfd, BLK, 0)
                finally:
                    feeder.join()
                    os.close(r)
            else:
                with open(fi, "rb") as a:
                    rc = D.deflate_compress(a.fileno(), b.fileno(), sfd, BLK, 0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return rc, fo.read_bytes(), fs.read_bytes()


def test_bgzf_file_path(tmp_path, enc):
    n = (3 << 20) + 17
    data = (D.gen_text(2 << 20, 8).tobytes() + D.gen_random(1 << 20, 9).tobytes() + D.gen_text(17, 10).tobytes())
    assert len(data) == n
    mem, _ = enc.compress_bytes(data, flags=D.DMX_BGZF)
    base = {"DMX_FORMAT": "bgzf", "DMX_CHUNK_MB": "1", "DMX_DEVICES": ""}
    rc, z, _ = _fd(tmp_path, data, base)
    assert rc == 0 and z == mem and gzip.decompress(z) == data
    assert z.endswith(EOF_MEMBER) and z.count(EOF_MEMBER) == 1
    rc, zp, _ = _fd(tmp_path, data, base, pipe_in=True)
    assert rc == 0 and zp == z
    # two workers on the one GPU
    fi, fo = tmp_path / "in", tmp_path / "multi"
    devs = (ctypes.c_int * 2)(0, 0)
    o = D.Opts(BLK, 0, D.DMX_BGZF, 0)
    with open(fi, "rb") as a, open(fo, "wb") as b:
        rc = D.lib().dmx_encode_fd_multi(a.fileno(), b.fileno(), ctypes.byref(o), 1 << 20, devs, 2)
    assert rc == 0 and fo.read_bytes() == z
    # with the records: the stream is the same, the tokens are the zlib stream's
    rc, zs, rec = _fd(tmp_path, data, base, stats=True)
    assert rc == 0 and zs == z
    rc, zz, recz = _fd(tmp_path, data, dict(base, DMX_FORMAT="zlib"), stats=True)
    assert rc == 0 and zlib.decompress(zz) == data and rec == recz and len(rec) > 0
