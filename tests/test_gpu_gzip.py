"""gzip container (DMX_F_GZIP) on the MI355X: the CRC-32 kernels against zlib.crc32 at every
size around the lane slice and the span, with unaligned bases; the gzip encode byte for byte
(gzip header + the oracle's DEFLATE data + CRC-32 / ISIZE) under every launch shape; the
output bound; shards; the file path; the block-index inflate; no flag state left behind."""
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

HDR10 = bytes([0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0, 0xFF])
BLK = 32768


@pytest.fixture(scope="module")
def enc():
    e = D.Encoder(0, 2 << 20)
    yield e
    e.close()


def _crc_sizes():
    S, L = D.crc32_geometry()
    return [0, 1, 2, 3, 4, 5, 15, 16, 17, L - 1, L, L + 1, S - 1, S, S + 1, 2 * S + 3, 5 * S + L + 1, (1 << 20) + 7]


def test_crc32_kernel_vs_zlib(enc):
    sizes = _crc_sizes()
    top = max(sizes)
    rng = np.random.default_rng(32)
    hosts = {"random": rng.integers(0, 256, top, dtype=np.uint8), "zeros": np.zeros(top, np.uint8),
             "ff": np.full(top, 0xFF, np.uint8)}
    for kind, h in hosts.items():
        base = torch.empty(top + 256 + 16, dtype=torch.uint8, device="cuda")
        a0 = (-base.data_ptr()) % 256   # a 256-byte aligned start inside the tensor
        for off in (0, 1, 3, 15):
            t = base[a0 + off:a0 + off + top]
            assert t.data_ptr() % 256 == off
            t.copy_(torch.from_numpy(h))
            hb = h.tobytes()
            for n in sizes:
                assert enc.crc32(t[:n]) == zlib.crc32(hb[:n]), (kind, off, n)


def test_crc32_async_on_empty_and_result_word(enc):
    w = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert enc._L.dmx_crc32_async(enc._ctx, None, 0, ctypes.c_void_p(w.data_ptr()), None) == 0   # the context's stream
    torch.cuda.synchronize()
    assert w.cpu().tolist() == [0, 0x5A5A5A5A]   # n == 0 gives 0; one word written


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


@functools.lru_cache(maxsize=None)
def _oracle(kind: str, n: int, fast: bool = False, check: bool = False) -> bytes:
    d = _input(kind, n)
    if fast:
        return O.compress(d, max_chain=7, lazy=True, deep=True, store_check=True)
    return O.compress(d, store_check=check)


def _want(data: bytes, o: bytes) -> bytes:
    return HDR10 + o[2:-4] + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


@pytest.mark.parametrize("kind", ["text", "random", "zeros", "mixed"])
def test_gzip_encode_byte_identical(enc, kind):
    for n in SIZES:
        data = _input(kind, n)
        z, r = enc.compress_bytes(data, flags=D.DMX_GZIP)
        assert z == _want(data, _oracle(kind, n)), (kind, n)
        assert gzip.decompress(z) == data, (kind, n)
        assert r.adler == zlib.crc32(data) and r.out_len == len(z)


FAST = D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK


def test_gzip_mixed_store_check_and_fast_parse(enc):
    for n in SIZES:
        data = _input("mixed", n)
        z, _ = enc.compress_bytes(data, flags=D.DMX_GZIP | D.DMX_F_STORE_CHECK)
        assert z == _want(data, _oracle("mixed", n, check=True)), n
        assert gzip.decompress(z) == data
        z, _ = enc.compress_bytes(data, max_chain=7, flags=D.DMX_GZIP | FAST)
        assert z == _want(data, _oracle("mixed", n, fast=True)), n
        assert gzip.decompress(z) == data


@pytest.mark.parametrize("worklist", ["0", "list", "plain"])
@pytest.mark.parametrize("scan3", [0, 1])
def test_gzip_under_hook_shapes(worklist, scan3):
    e = D.Encoder(0, 1 << 20)   # a context of its own: the module's keeps its hooks
    try:
        e.set_hook("worklist", worklist)
        e.set_hook("scan3", scan3)
        for n in (0, 1, 32769, 5 * BLK + 1):
            data = _input("mixed", n)
            z, _ = e.compress_bytes(data, max_chain=7, flags=D.DMX_GZIP | FAST)
            assert z == _want(data, _oracle("mixed", n, fast=True)), (worklist, scan3, n)
            z, _ = e.compress_bytes(data, flags=D.DMX_GZIP | D.DMX_F_STORE_CHECK)
            assert z == _want(data, _oracle("mixed", n, check=True)), (worklist, scan3, n)
        rnd = _input("random", 5 * BLK + 1)   # all stored: the whole-copy prefix behind the 10-byte header
        for _ in range(2):   # (the second encode runs with the first one's launch-shape hint)
            z, _ = e.compress_bytes(rnd, max_chain=7, flags=D.DMX_GZIP | FAST)
            assert z == _want(rnd, O.compress(rnd, max_chain=7, lazy=True, deep=True, store_check=True))
    finally:
        e.set_hook("worklist", None)
        e.set_hook("scan3", 0)
        e.close()


def test_gzip_capacity(enc):
    n = 3 * BLK
    data = _input("random", n)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    o = D.Opts(BLK, 0, D.DMX_GZIP, 0)
    cap = D.max_compressed(n, BLK, D.DMX_GZIP)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    enc.reserve(n, BLK)
    torch.cuda.synchronize()   # (the encodes below run on the context's own stream)
    enc.encode_async(t.data_ptr(), n, out.data_ptr(), cap, None, o)
    r = enc.result()
    z = out[:r.out_len].cpu().numpy().tobytes()
    assert r.out_len == 10 + 3 * (BLK + 5) + 8 and gzip.decompress(z) == data
    rounded = (r.out_len + 3) & ~3
    enc.encode_async(t.data_ptr(), n, out.data_ptr(), rounded, None, o)   # exactly enough
    assert enc.result().out_len == r.out_len
    enc.encode_async(t.data_ptr(), n, out.data_ptr(), rounded - 4, None, o)
    with pytest.raises(D.DeflateError) as ei:
        enc.result()
    assert ei.value.code == -D.E["E_SZ"]


def test_gzip_shards(enc):
    n = 4 * BLK + 100
    data = _input("text", n)
    cuts = [0, BLK, 3 * BLK, n]
    pieces, crcs, lens = [], [], []
    for k in range(3):
        part = data[cuts[k]:cuts[k + 1]]
        z, r = enc.compress_bytes(part, flags=shard.shard_flags(k, 3) | D.DMX_F_GZIP)
        pieces.append(z)
        crcs.append(r.adler)
        lens.append(len(part))
        assert r.adler == zlib.crc32(part)   # reported without DMX_F_TRAILER
    assert pieces[0][:10] == HDR10
    z = b"".join(pieces) + shard.trailer_gzip(shard.combine_crc32(crcs, lens), n)
    assert gzip.decompress(z) == data


def _fd_gzip(tmp_path, data: bytes, env: dict, pipe_in: bool = False):
    fi, fo = tmp_path / "in", tmp_path / "out"
    fi.write_bytes(data)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with open(fo, "wb") as b:
            if pipe_in:
                r, w = os.pipe()
                feeder = threading.Thread(target=lambda: (os.write(w, data), os.close(w)))
                feeder.start()
                try:
                    rc = D.deflate_compress(r, b.fileno(), -1, BLK, 0)
                finally:
                    feeder.join()
                    os.close(r)
            else:
                with open(fi, "rb") as a:
                    rc = D.deflate_compress(a.fileno(), b.fileno(), -1, BLK, 0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return rc, fo.read_bytes()


FAST_ENV = {"DMX_MAX_CHAIN": "7", "DMX_LAZY": "1", "DMX_DEEP": "1", "DMX_STORE_CHECK": "1"}


def test_gzip_file_path(tmp_path):
    n = (3 << 20) + 17
    data = (D.gen_text(2 << 20, 8).tobytes() + D.gen_random(1 << 20, 9).tobytes() + D.gen_text(17, 10).tobytes())
    assert len(data) == n
    base = {"DMX_FORMAT": "gzip", "DMX_CHUNK_MB": "1", "DMX_DEVICES": ""}
    rc, z = _fd_gzip(tmp_path, data, base)
    assert rc == 0 and z[:10] == HDR10 and gzip.decompress(z) == data
    assert z[-8:] == struct.pack("<II", zlib.crc32(data), n)
    rc, zf = _fd_gzip(tmp_path, data, dict(base, **FAST_ENV))
    assert rc == 0 and gzip.decompress(zf) == data
    rc, zp = _fd_gzip(tmp_path, data, base, pipe_in=True)
    assert rc == 0 and gzip.decompress(zp) == data
    # unset / "zlib": today's stream
    rc, zz = _fd_gzip(tmp_path, data, dict(base, DMX_FORMAT="zlib"))
    assert rc == 0 and zlib.decompress(zz) == data and zz[2:-4] == z[10:-8]
    # two workers on the one GPU
    fi, fo = tmp_path / "in", tmp_path / "multi"
    devs = (ctypes.c_int * 2)(0, 0)
    o = D.Opts(BLK, 0, D.DMX_F_GZIP, 0)
    with open(fi, "rb") as a, open(fo, "wb") as b:
        rc = D.lib().dmx_encode_fd_multi(a.fileno(), b.fileno(), ctypes.byref(o), 1 << 20, devs, 2)
    assert rc == 0 and fo.read_bytes() == z


def test_gzip_block_index_inflate(enc):
    n = 2 * BLK + 12345
    data = _input("text", n)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    out, r = enc.compress_tensor(t, opts=D.Opts(BLK, 0, D.DMX_GZIP, 0))
    assert r.nblocks == 3 and out[:10].cpu().numpy().tobytes() == HDR10
    ix, nb = enc.block_index()
    dec, st = D.inflate_gpu(out, n, ix, nb)
    assert st == 0 and dec.cpu().numpy().tobytes() == data
    # stream-mode GPU inflate of a gzip member is out of scope: its header error, no output
    dec, st = D.inflate_gpu(out, n + 16)
    assert st != 0


def test_zlib_after_gzip_same_context(enc):
    data = _input("mixed", 5 * BLK + 1)
    z, _ = enc.compress_bytes(data, max_chain=7, flags=D.DMX_GZIP | FAST)
    assert z[:10] == HDR10
    z, r = enc.compress_bytes(data, max_chain=7, flags=D.DMX_ZLIB | FAST)
    assert z == _oracle("mixed", 5 * BLK + 1, fast=True)
    assert r.adler == zlib.adler32(data)
    z, r = enc.compress_bytes(b"", flags=D.DMX_ZLIB)
    assert z == O.compress(b"") and zlib.decompress(z) == b""


def test_gzip_empty_on_context_without_workspace():
    """A context that never reserved a block (max_input 0) has no CRC scratch: an empty gzip
    encode needs none and gives the 20-byte member, as the zlib path gives its 8 bytes; a CRC
    of real bytes on it is -E_SZ until the context is reserved."""
    e = D.Encoder(0, 0)
    try:
        out = torch.zeros(64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()   # (the context's own stream below)
        for flags, want in ((D.DMX_GZIP, HDR10 + b"\x03\x00" + bytes(8)), (D.DMX_ZLIB, O.compress(b""))):
            e.encode_async(out.data_ptr(), 0, out.data_ptr(), 64, None, D.Opts(BLK, 0, flags, 0))
            r = e.result()
            assert out[:r.out_len].cpu().numpy().tobytes() == want
        assert gzip.decompress(HDR10 + b"\x03\x00" + bytes(8)) == b""
        assert r.adler == 1   # the zlib encode after the gzip one reports Adler-32 again
        w = torch.zeros(1, dtype=torch.int32, device="cuda")
        t = torch.zeros(100, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = e._L.dmx_crc32_async(e._ctx, ctypes.c_void_p(t.data_ptr()), 100, ctypes.c_void_p(w.data_ptr()), None)
        assert rc == -D.E["E_SZ"]
        assert e.crc32(t) == zlib.crc32(bytes(100))   # (reserves first)
        z, _ = e.compress_bytes(b"", flags=D.DMX_GZIP)
        assert gzip.decompress(z) == b""
    finally:
        e.close()


@pytest.mark.parametrize("n", [0, 1, 1000, 3 * BLK + 17])
def test_compress_host_buffer_gzip(n):
    """dmx_encode_host under DMX_F_GZIP (compress(gzip=True)): sized by the gzip bound."""
    data = _input("mixed", n)
    z = D.compress(data, gzip=True)
    assert z == _want(data, _oracle("mixed", n)) and gzip.decompress(z) == data
    assert D.compress(data, flags=D.DMX_GZIP, max_chain=7, lazy=True, deep=True, store_check=True) == \
        _want(data, _oracle("mixed", n, fast=True))
    assert D.compress(data) == _oracle("mixed", n)   # and zlib on the same cached context after it
