"""Inputs for the range-read tests (test_gpu_bgzf_ranges.py): BGZF members with a longer header than
bgzf_read_inputs.member writes, and the expectations that Python slicing gives.  zlib / gzip are the
judge of every file made here."""
import gzip
import struct
import zlib

from bgzf_read_inputs import EOF_MEMBER


def member_named(block: bytes, level: int, name: bytes = b"reads.bam") -> bytes:
    """block as a BGZF member whose FEXTRA field holds another subfield before "BC" (XLEN 14) and
    whose header goes on with FNAME: the DEFLATE data begins 12 + XLEN + len(name) + 1 bytes in"""
    c = zlib.compressobj(level, wbits=-15)
    d = c.compress(block) + c.flush()
    size = 12 + 14 + len(name) + 1 + len(d) + 8
    assert size <= 65536
    h = (bytes([0x1F, 0x8B, 0x08, 0x04 | 0x08, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", 14)
         + b"XY" + struct.pack("<H", 4) + b"\x01\x02\x03\x04" + b"BC" + struct.pack("<HH", 2, size - 1) + name + b"\0")
    return h + d + struct.pack("<II", zlib.crc32(block), len(block))


def named_file(data: bytes, sizes, level: int):
    """bgzf_read_inputs.bgzf_file with member_named: (file, [(member offset, member size, data offset, ISIZE)])"""
    assert sum(sizes) == len(data)
    out, lay, o, p = [], [], 0, 0
    for n in sizes:
        m = member_named(data[o:o + n], level)
        out.append(m)
        lay.append((p, len(m), o, n))
        o += n
        p += len(m)
    z = b"".join(out) + EOF_MEMBER
    assert gzip.decompress(z) == data
    return z, lay


def want_bytes(data: bytes, ranges):
    """[data[off:off + len]] as pread clips them"""
    return [data[off:off + ln] for off, ln in ranges]


def want_members(lay, data: bytes, ranges) -> int:
    """the members with data that some non-empty clipped range touches"""
    total, hit = len(data), set()
    for off, ln in ranges:
        lo, hi = min(off, total), min(off + ln, total)
        if lo < hi:
            hit.update(k for k, (_, _, o, n) in enumerate(lay) if n and o < hi and lo < o + n)
    return len(hit)
