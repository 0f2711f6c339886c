"""Inputs of test_inflate_multi_api.py and test_gpu_inflate_multi.py (one .gz file of many members,
RFC 1952 2.2): files of Python's zlib members over synthetic text, hand-built members
(deflate_craft) whose headers straddle chunk boundaries or hide a second header, a stored block
that carries a whole member, members with a match that reaches before their own first byte, and
trailing or broken ends.  The reference everywhere is reference(): a zlib.decompressobj(31) loop
over unused_data, continued while the rest begins 1F 8B.  All files are under 1 MB.  Built once per
process."""
import gzip
import struct
import zlib

import deflate_compression_amd as D
import deflate_craft as C
from inflate_parallel_inputs import _apply, _block, deflate

CHUNK = 1024
E = D.E
_cache = {}


def text():
    if "text" not in _cache:
        _cache["text"] = D.gen_text(700_000, 11).tobytes()
    return _cache["text"]


def member(data, raw=None, level=6, flush_every=0, strategy=zlib.Z_DEFAULT_STRATEGY, extra=None, name=None, comment=None,
           hcrc=False, crc=None, isize=None):
    """one gzip member around `raw` (default: zlib's raw DEFLATE of data), with any header fields"""
    if raw is None:
        raw = deflate(data, level, -15, strategy, flush_every)
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | \
        (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\x00\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    c = zlib.crc32(data) if crc is None else crc
    n = len(data) if isize is None else isize
    return h + raw + struct.pack("<II", c & 0xFFFFFFFF, n & 0xFFFFFFFF)


def reference(z):
    """[(in_off, out_len, crc32, data)] per member by zlib, and in_used; raises zlib.error as zlib does"""
    out, pos = [], 0
    while True:
        d = zlib.decompressobj(31)
        data = d.decompress(z[pos:])
        if not d.eof:
            raise zlib.error("incomplete member")
        out.append((pos, len(data), zlib.crc32(data), data))
        pos = len(z) - len(d.unused_data)
        if z[pos:pos + 2] != b"\x1f\x8b":
            return out, pos


def two_sync():
    if "two" not in _cache:
        t = text()
        a = member(t[:60_000], flush_every=3000)
        b = member(t[60_000:120_000], flush_every=3000, extra=b"AB\x04\x00wxyz", name=b"second.txt", comment=b"a comment",
                   hcrc=True)
        _cache["two"] = (a, b)
    return _cache["two"]


def small_300():
    if "small" not in _cache:
        t = text()
        parts, pos = [], 0
        for k in range(300):
            n = 700 + (k * 977) % 2301
            d = t[pos:pos + n]
            pos += n
            kind = k % 5
            if kind == 3:
                parts.append(member(d, level=0))
            elif kind == 4:
                parts.append(member(d, strategy=zlib.Z_FIXED))
            else:
                parts.append(member(d, level=(1, 6, 9)[kind]))
        _cache["small"] = b"".join(parts)
    return _cache["small"]


def empties():
    t = text()
    e = gzip.compress(b"")
    return e + member(t[:6000], flush_every=1500) + e + e + member(t[6000:11_000], flush_every=1500) + e


def header_straddle():
    """member 0 is text; member 1's FEXTRA is padded so that its header spans a chunk boundary and
    holds, first in the next chunk, ten bytes that read as a member header in front of a stored
    block (a false member start whose walk fails); member 2's FEXTRA ends at a chunk boundary, where
    its FNAME begins with 1F 8B 08 08, a date and a name of its own -- a header that ends with the
    real name's terminator, so the false member's body is the real one's."""
    if "straddle" not in _cache:
        t = text()
        z = member(t[:3000], flush_every=1000)
        fake = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + bytes(8)
        to_edge = -(len(z) + 12) % CHUNK   # the extra field's bytes in front of the boundary
        z += member(t[3000:7000], flush_every=1000, extra=b"P" * to_edge + fake + b"Q" * 40)
        to_edge = -(len(z) + 12) % CHUNK
        inner = b"\x1f\x8b\x08\x08\x01\x01\x01\x01\x02\x03inner-name"
        start = len(z)
        z += member(t[7000:12_000], flush_every=1000, extra=b"R" * to_edge, name=inner)
        assert (start + 12 + to_edge) % CHUNK == 0 and z[start + 12 + to_edge:start + 16 + to_edge] == inner[:4]
        z += member(t[12_000:14_000])
        _cache["straddle"] = z
    return _cache["straddle"]


def nested():
    """a stored block whose payload holds a complete small member at byte 1024 of the file, first in
    its chunk: a member start that is none of this file's"""
    t = text()
    inner = member(t[50_000:50_600])
    pad = CHUNK - 15   # header 10, the stored block's 5
    payload = t[:pad] + inner + t[pad:pad + 100]
    raw = C.Deflate().stored(payload, False).getvalue() + deflate(t[1200:9000], 6, -15, flush_every=1500)
    data = payload + t[1200:9000]
    z = member(data, raw=raw)
    assert z[CHUNK:CHUNK + 3] == b"\x1f\x8b\x08"
    return z + member(t[9000:12_000], flush_every=1000)


def five_mib_zeros():
    if "zeros" not in _cache:
        t = text()
        _cache["zeros"] = member(t[:20_000], flush_every=3000) + member(bytes(5 << 20)) + member(t[20_000:40_000], flush_every=3000)
    return _cache["zeros"]


def single():
    return member(text()[:60_000], flush_every=3000)


def well_formed():
    """[(name, file)]: the files zlib and gzip.decompress read to their end"""
    a, b = two_sync()
    return [("two-sync", a + b), ("small-300", small_300()), ("empties", empties()), ("header-straddle", header_straddle()),
            ("nested", nested()), ("single", single())]


def trailing():
    """[(name, file)]: two-sync with trailing data, which is ignored: in_used is the members' end"""
    a, b = two_sync()
    return [("junk-behind", a + b + b"junk"), ("zeros-behind", a + b + bytes(100)), ("lone-1f", a + b + b"\x1f")]


def broken():
    """[(name, file, plan status (None: the host plan's own), decode status, bad_member)]: two-sync with a
    broken end; the last two are clean for the plan and for a decode without verify"""
    a, b = two_sync()
    z = a + b
    crc = bytearray(z)
    crc[-8] ^= 0x10
    isz = bytearray(z)
    isz[-4] ^= 0x01
    return [("magic-only", z + b"\x1f\x8b", -E["E_ZHEAD"], -E["E_ZHEAD"], None),
            ("method-7", z + b"\x1f\x8b\x07\x00\x00\x00\x00\x00\x00\x03", -E["E_ZCMPMT"], -E["E_ZCMPMT"], None),
            ("cut-trailer", z[:-3], -E["E_CRC"], -E["E_CRC"], None),
            ("cut-block", z[:len(a) + len(b) // 2], None, None, None),
            ("crc-flip", bytes(crc), 0, -E["E_CRC"], 1),
            ("isize-flip", bytes(isz), 0, -E["E_LEN"], 1)]


def _far_member(tokens_per_block, nblocks, bad_block, bad_tokens):
    """a member of `nblocks` dynamic blocks of literals from the text, block `bad_block` beginning with
    `bad_tokens` instead; returns (member, the bit inside the member's DEFLATE data where that block begins)"""
    t = text()
    d = C.Deflate()
    out = bytearray()
    bad_bit = None
    for k in range(nblocks):
        toks = list(t[200_000 + k * tokens_per_block:200_000 + (k + 1) * tokens_per_block])
        if k == bad_block:
            bad_bit = d.bitpos
            toks = bad_tokens(len(out)) + toks
        _block(d, toks, final=k == nblocks - 1)
        try:
            _apply(toks, out)
        except IndexError:
            out += bytes(8)   # (the bad match has no source: the bytes do not matter)
    return member(bytes(out), raw=d.getvalue()), bad_bit


def far_files():
    """[(name, file, offset of member 1, bit of the bad block in the file)]: member 1 has a match whose
    source begins one byte (far-a, far-b) or three bytes and wholly (far-a-whole) before the member's
    first byte.  far-a: its first match, the member beginning inside a chunk; far-b: in a block 6 000
    bytes into a member of many blocks, which a later live chunk starts with."""
    if "far" not in _cache:
        t = text()
        first = member(t[:3000])
        assert len(first) % CHUNK > 64
        out = []
        for name, nb, bad, mk in (("far-a", 2, 0, lambda pos: list(b"0123456789") + [(5, pos + 11)]),
                                  ("far-a-whole", 2, 0, lambda pos: list(b"0123456789") + [(3, pos + 13)]),
                                  ("far-b", 8, 3, lambda pos: list(b"0123456789") + [(5, pos + 11)])):
            m, bit = _far_member(2000, nb, bad, mk)
            out.append((name, first + m, len(first), 8 * (len(first) + 10) + bit))
        _cache["far"] = out
    return _cache["far"]
