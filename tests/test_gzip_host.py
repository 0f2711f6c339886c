"""gzip container (RFC 1952), host side, no GPU: the CRC-32 combine against zlib.crc32, the host
inflate of gzip members (optional header fields, error codes, truncation), the shard helpers,
the output bound, and DMX_FORMAT validation in deflate_compress."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import deflate_compression_amd as D
from deflate_compression_amd import shard


def test_crc32_combine_random_pairs():
    rng = np.random.default_rng(1952)
    lens_b = [0, 0, 1, 5000] + [int(x) for x in rng.integers(0, 5001, 46)]
    assert len(lens_b) == 50
    for k, lb in enumerate(lens_b):
        la = int(rng.integers(0, 5001)) if k != 1 else 0
        a = rng.integers(0, 256, la, dtype=np.uint8).tobytes()
        b = rng.integers(0, 256, lb, dtype=np.uint8).tobytes()
        assert D.crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)


def test_crc32_combine_associative():
    rng = np.random.default_rng(7)
    for _ in range(10):
        a, b, c = (rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 3000, 3))
        ca, cb, cc = zlib.crc32(a), zlib.crc32(b), zlib.crc32(c)
        left = D.crc32_combine(D.crc32_combine(ca, cb, len(b)), cc, len(c))
        right = D.crc32_combine(ca, D.crc32_combine(cb, cc, len(c)), len(b) + len(c))
        assert left == right == zlib.crc32(a + b + c)


def _crc_zeros(n: int) -> int:
    """CRC-32 of n zero bytes from small buffers and the combine (doubling)."""
    unit = 1 << 16
    crc, have = zlib.crc32(bytes(unit)), unit   # crc of `have` zero bytes, have = unit * 2^k
    rest = n % unit
    out = zlib.crc32(bytes(rest))
    out_len = rest
    m = n // unit
    while m:
        if m & 1:
            out = D.crc32_combine(out, crc, have)
            out_len += have
        crc = D.crc32_combine(crc, crc, have)
        have *= 2
        m >>= 1
    assert out_len == n
    return out


def test_crc32_combine_len_past_2_32():
    """len_b = 2^33 + 5, checked against the operator's own definition: (a, b || c) must equal
    ((a, b), c) with zero-filled pieces whose CRCs come from small buffers plus combine."""
    assert _crc_zeros(200000) == zlib.crc32(bytes(200000))   # the doubling helper itself
    a = b"the quick brown fox"
    ca = zlib.crc32(a)
    lb, lc = (1 << 33) - 1000, 1005
    assert lb + lc == (1 << 33) + 5
    cb, cc = _crc_zeros(lb), _crc_zeros(lc)
    cbc = D.crc32_combine(cb, cc, lc)
    assert cbc == _crc_zeros(lb + lc)
    whole = D.crc32_combine(ca, cbc, lb + lc)
    steps = D.crc32_combine(D.crc32_combine(ca, cb, lb), cc, lc)
    assert whole == steps
    # a third route, the order of x (2^32 - 1): a shift by 8 len bits is one by 8 len mod
    # (2^32 - 1) bits, here 2^36 + 40 = 56 bits = 7 bytes
    short = (8 * (lb + lc)) % ((1 << 32) - 1)
    assert short == 56
    assert D.crc32_combine(ca, 0, lb + lc) == D.crc32_combine(ca, 0, short // 8)


def _text(n, seed=3):
    return D.gen_text(n, seed).tobytes() if n else b""


@pytest.mark.parametrize("n", [0, 1, 100, 70000])
@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_inflate_gzip_members(n, level):
    d = _text(n)
    z = gzip.compress(d, compresslevel=level, mtime=0)
    assert z[:2] == b"\x1f\x8b"
    assert D.deflate_decompress(z) == d
    assert D.deflate_decompress(z + b"trailing garbage") == d   # one member; the rest ignored


FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


def _member(data: bytes, flg: int = 0, cm: int = 8) -> bytes:
    """A hand-built gzip member with the optional fields FLG selects."""
    h = bytes([0x1F, 0x8B, cm, flg]) + struct.pack("<IBB", 0, 0, 255)
    if flg & FEXTRA:
        extra = b"AB\x03\x00xyz"
        h += struct.pack("<H", len(extra)) + extra
    if flg & FNAME:
        h += b"file.txt\x00"
    if flg & FCOMMENT:
        h += b"a comment\x00"
    if flg & FHCRC:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush()
    return h + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


ALL_FIELDS = FTEXT | FHCRC | FEXTRA | FNAME | FCOMMENT


@pytest.mark.parametrize("flg", [FEXTRA, FNAME, FCOMMENT, FHCRC, ALL_FIELDS])
def test_inflate_gzip_optional_fields(flg):
    d = _text(5000, 5)
    z = _member(d, flg)
    assert gzip.decompress(z) == d   # the hand-built member is a valid one
    assert D.deflate_decompress(z) == d


def test_inflate_gzip_nullterm():
    d = _text(1234, 9)
    out = D.deflate_decompress(gzip.compress(d, mtime=0), D.DEFLATE_NULLTERM)
    assert out == d + b"\0"


def _code(z) -> int:
    with pytest.raises(D.DeflateError) as ei:
        D.deflate_decompress(z)
    return ei.value.code


def test_inflate_gzip_error_codes():
    d = _text(3000, 11)
    z = bytearray(gzip.compress(d, mtime=0))
    bad = bytearray(z)
    bad[-8] ^= 0x01   # CRC-32
    assert _code(bad) == -D.E["E_CRC"]
    bad = bytearray(z)
    bad[-1] ^= 0x80   # ISIZE
    assert _code(bad) == -D.E["E_LEN"]
    assert _code(_member(d, 0, cm=7)) == -D.E["E_ZCMPMT"]
    for bit in (0x20, 0x40, 0x80):
        assert _code(_member(d, bit)) == -D.E["E_RESERV"]
    # a zlib stream still answers with its own codes
    zz = bytearray(zlib.compress(d))
    zz[-1] ^= 1
    assert _code(zz) == -D.E["E_ZADL32"]


def test_inflate_gzip_every_prefix_fails():
    d = _text(300, 13)
    z = _member(d, ALL_FIELDS)
    assert D.deflate_decompress(z) == d
    for k in range(len(z)):
        with pytest.raises(D.DeflateError):
            D.deflate_decompress(z[:k])
    # the header cut short is -E_ZHEAD, the trailer cut short -E_CRC
    assert _code(z[:9]) == -D.E["E_ZHEAD"]
    assert _code(z[:15]) == -D.E["E_ZHEAD"]
    assert _code(z[:-1]) == -D.E["E_CRC"]
    assert _code(z[:-8]) == -D.E["E_CRC"]


def test_shard_crc_helpers():
    rng = np.random.default_rng(3)
    parts = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in (0, 1, 32768, 65536 + 100, 17)]
    whole = b"".join(parts)
    crc = shard.combine_crc32([zlib.crc32(p) for p in parts], [len(p) for p in parts])
    assert crc == zlib.crc32(whole)
    assert shard.trailer_gzip(crc, len(whole)) == struct.pack("<II", zlib.crc32(whole), len(whole))
    assert shard.trailer_gzip(0xFFFFFFFF, (1 << 32) + 7) == struct.pack("<II", 0xFFFFFFFF, 7)
    assert shard.combine_crc32([], []) == 0
    # the existing helpers keep their defaults
    assert shard.trailer(0x01020304) == b"\x01\x02\x03\x04"
    assert shard.combine_adler([zlib.adler32(p) for p in parts], [len(p) for p in parts]) == zlib.adler32(whole)


def test_max_compressed_gzip_bound():
    assert D.DMX_F_GZIP == 512 and D.DMX_GZIP == D.DMX_ZLIB | D.DMX_F_GZIP
    for n in (0, 1, 32767, 32768, 32769, 100000, 1 << 30):
        assert D.max_compressed(n, 32768, D.DMX_GZIP) == D.max_compressed(n) + 12
        assert D.max_compressed(n, 32768, D.DMX_ZLIB) == D.max_compressed(n) == D.max_compressed(n, 32768)
    assert D.max_compressed(5000, 1024, D.DMX_GZIP) == D.max_compressed(5000, 1024) + 12


def test_crc32_geometry():
    span, lane = D.crc32_geometry()
    assert lane >= 16 and span % lane == 0 and span // lane >= 64


def test_bad_format_fails_before_encoding(tmp_path, monkeypatch):
    """An unknown DMX_FORMAT value is rejected with -E_INVAL before anything is read, encoded
    or written (no GPU needed: the check comes first)."""
    monkeypatch.setenv("DMX_FORMAT", "bogus")
    fi, fo = tmp_path / "in", tmp_path / "out"
    fi.write_bytes(b"hello hello hello")
    a = os.open(fi, os.O_RDONLY)
    b = os.open(fo, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        assert D.deflate_compress(a, b, -1, 32768, 0) == -D.E["E_INVAL"]
        assert os.lseek(a, 0, os.SEEK_CUR) == 0
    finally:
        for x in (a, b):
            os.close(x)
    assert fo.read_bytes() == b""
