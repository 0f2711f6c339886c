"""BGZF files as writers other than this project make them, for the reader's tests
(test_bgzf_read_host.py, test_gpu_bgzf_read.py): members of any size the format allows, each the
raw DEFLATE data of Python's zlib behind the 18-byte header, before CRC-32 and ISIZE.  zlib is the
judge of every file made here: a member is at most 65 536 bytes and gzip.decompress gives the data."""
import gzip
import struct
import zlib

import numpy as np

HDR16 = bytes([0x1F, 0x8B, 0x08, 0x04, 0, 0, 0, 0, 0, 0xFF, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00])
EOF_MEMBER = HDR16 + bytes([0x1B, 0x00, 0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0])
HTS = 65280     # htslib's block: 64 KiB less 256, so that a stored member still fits BSIZE
TOP = 65536     # the largest ISIZE the format allows


def wrap(deflate: bytes, block: bytes) -> bytes:
    """the BGZF member around the raw DEFLATE data of block"""
    size = 18 + len(deflate) + 8
    assert size <= 65536, (len(block), size)
    return HDR16 + struct.pack("<H", size - 1) + deflate + struct.pack("<II", zlib.crc32(block), len(block))


def member(block: bytes, level: int) -> bytes:
    """block as one BGZF member (ISIZE = len(block); an empty block is an empty member)"""
    c = zlib.compressobj(level, wbits=-15)
    return wrap(c.compress(block) + c.flush(), block)


def bgzf_file(data: bytes, sizes, level: int, eof: bool = True):
    """(file, [(member offset, member size, data offset, ISIZE)]): data cut into members of the
    given ISIZEs (which sum to len(data); 0 = an empty member), then the end-of-file member"""
    assert sum(sizes) == len(data)
    out, lay, o, p = [], [], 0, 0
    for n in sizes:
        m = member(data[o:o + n], level)
        out.append(m)
        lay.append((p, len(m), o, n))
        o += n
        p += len(m)
    z = b"".join(out) + (EOF_MEMBER if eof else b"")
    assert gzip.decompress(z) == data if z else data == b""
    return z, lay


def hts_sizes(n: int):
    """the ISIZEs of n bytes as htslib cuts them: 65 280 each, then the rest"""
    return [HTS] * (n // HTS) + ([n % HTS] if n % HTS else [])


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
          8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
_CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def deflate_matches(raw: bytes):
    """[(output position, length, distance)] of every match of a raw DEFLATE stream (RFC 1951), read
    bit by bit in plain Python: what a compressor really emitted, without the code under test"""
    pos = [0]

    def bits(n):
        v = 0
        for k in range(n):
            v |= ((raw[pos[0] >> 3] >> (pos[0] & 7)) & 1) << k
            pos[0] += 1
        return v

    def table(lens):
        code, out = 0, {}
        for ln in range(1, 16):
            for s, l in enumerate(lens):
                if l == ln:
                    out[(ln, code)] = s
                    code += 1
            code <<= 1
        return out

    def sym(t):
        code = 0
        for ln in range(1, 16):
            code = (code << 1) | bits(1)
            if (ln, code) in t:
                return t[(ln, code)]
        raise ValueError("no code")

    out, op, last = [], 0, 0
    while not last:
        last, bt = bits(1), bits(2)
        if bt == 0:
            pos[0] = (pos[0] + 7) & ~7
            n = bits(16)
            bits(16)
            pos[0] += 8 * n
            op += n
            continue
        if bt == 1:
            tl, td = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 30)
        else:
            assert bt == 2
            hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
            cl = [0] * 19
            for k in range(hclen):
                cl[_CLORDER[k]] = bits(3)
            tc, lens = table(cl), []
            while len(lens) < hlit + hdist:
                s = sym(tc)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + bits(2))
                else:
                    lens += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
            tl, td = table(lens[:hlit]), table(lens[hlit:])
        while True:
            s = sym(tl)
            if s < 256:
                op += 1
            elif s == 256:
                break
            else:
                ln = _LBASE[s - 257] + bits(_LEXT[s - 257])
                d = sym(td)
                out.append((op, ln, _DBASE[d] + bits(_DEXT[d])))
                op += ln
    return out


def entries(idx: np.ndarray):
    """[(bit, out_off, out_len)] of a dmx_iblock array"""
    a = idx.view(np.uint64).reshape(-1, 3)
    return [(int(r[0]), int(r[1]), int(r[2] & 0xFFFFFFFF)) for r in a]


def want_entries(lay):
    """the entries dmx_bgzf_index_max must give for a layout: members with data only"""
    return [(8 * (p + 18), o, n) for p, _, o, n in lay if n]
