"""ZIP archives for the tests of the ZIP index and decode: a hand writer (craft) for the shapes
zipfile does not write -- ZIP64 extras with markers, prefixes, comments, data descriptors with zeroed
local fields, local extras the central directory lacks, bytes inside the directory that parse as
headers -- and archives written by zipfile itself.  CPython's zipfile opens every archive of
CASES, testzip() is clean and the bytes come back (test_zip_api.py checks it), so zipfile is the
reference for the index and for the decoded bytes."""
import functools
import io
import struct
import zipfile
import zlib

import numpy as np

import deflate_compression_amd as D

M32 = 0xFFFFFFFF


def text(n: int, seed: int) -> bytes:
    return D.gen_text(max(n, 1), seed).tobytes()[:n]


def noise(n: int, seed: int) -> bytes:
    return D.gen_random(max(n, 1), seed).tobytes()[:n]


def raw_deflate(data: bytes, level: int = 6, strategy: int = 0) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def three_blocks(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    a = len(data) // 3
    return c.compress(data[:a]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[a:2 * a]) + c.flush(zlib.Z_FULL_FLUSH) + \
        c.compress(data[2 * a:]) + c.flush()


class Ent:
    """one entry for craft: comp = the payload as stored in the file (default: data deflated, or data
    itself for method 0); z64 = the fields that carry the 0xFFFFFFFF marker and live in the ZIP64 extra"""

    def __init__(self, name, data=b"", method=8, comp=None, cextra=b"", lextra=b"", fcomment=b"", z64=(), flags=0):
        self.name = name.encode() if isinstance(name, str) else name
        self.data = data
        self.method = method
        self.comp = comp if comp is not None else (raw_deflate(data) if method == 8 else data)
        self.cextra, self.lextra, self.fcomment = cextra, lextra, fcomment
        self.z64 = set(z64)
        self.flags = flags


def craft(entries, zip64=False, comment=b"", prefix=b"", dd=False, local_extra=b"", tail64=None):
    """The bytes of an archive of `entries`.  zip64: every entry carries all three markers and the
    ZIP64 end record and locator are written (tail64 overrides the latter alone).  dd: data
    descriptors, with CRC and sizes zeroed in the local headers.  local_extra: an extra field every
    local header has and the central directory lacks.  Stored offsets do not count `prefix`."""
    body = bytearray()
    central = bytearray()
    for e in entries:
        z64 = {"usize", "csize", "off"} if zip64 else e.z64
        crc = zlib.crc32(e.data) & M32
        flags = e.flags | (8 if dd else 0)
        off = len(body)
        lx = e.lextra + local_extra
        body += struct.pack("<IHHHHHIIIHH", 0x04034B50, 45 if z64 else 20, flags, e.method, 0, 0x21, 0 if dd else crc,
                            0 if dd else len(e.comp), 0 if dd else len(e.data), len(e.name), len(lx))
        body += e.name + lx + e.comp
        if dd:
            body += struct.pack("<IIII", 0x08074B50, crc, len(e.comp), len(e.data))
        x64 = b""
        if "usize" in z64:
            x64 += struct.pack("<Q", len(e.data))
        if "csize" in z64:
            x64 += struct.pack("<Q", len(e.comp))
        if "off" in z64:
            x64 += struct.pack("<Q", off)
        cx = (struct.pack("<HH", 1, len(x64)) + x64 if z64 else b"") + e.cextra
        central += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 45, 45 if z64 else 20, flags, e.method, 0, 0x21, crc,
                               M32 if "csize" in z64 else len(e.comp), M32 if "usize" in z64 else len(e.data), len(e.name),
                               len(cx), len(e.fcomment), 0, 0, 0, M32 if "off" in z64 else off)
        central += e.name + cx + e.fcomment
    cd_off, cd_size, n = len(body), len(central), len(entries)
    tail = bytearray()
    if zip64 if tail64 is None else tail64:
        tail += struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, n, n, cd_size, cd_off)
        tail += struct.pack("<IIQI", 0x07064B50, 0, cd_off + cd_size, 1)
        tail += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, min(n, 0xFFFF), min(n, 0xFFFF), M32, M32, len(comment))
    else:
        tail += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, n, n, cd_size, cd_off, len(comment))
    return bytes(prefix) + bytes(body) + bytes(central) + bytes(tail) + bytes(comment)


def small_entries(n: int, name_len: int = 0):
    out = []
    for i in range(n):
        nm = f"e{i:05d}"
        nm = nm + "_" * max(0, name_len - len(nm))
        d = (b"%d:" % i) * (1 + i % 5)
        out.append(Ent(nm, d, 8 if i % 3 else 0))
    return out


def fake_header(fill: int, n: int, m: int, k: int) -> bytes:
    """46 bytes that pass the central header step where 46 + n + m + k bytes follow in the directory"""
    return b"PK\x01\x02" + bytes([fill]) * 24 + struct.pack("<HHH", n, m, k) + bytes([fill]) * 14


def payload_entries():
    t70 = text(70 << 10, 7)
    return [
        Ent("empty_deflated", b"", 8, comp=b"\x03\x00"),
        Ent("empty_stored", b"", 0),
        Ent("one_byte", b"Z", 8),
        Ent("one_byte_stored", b"Q", 0),
        Ent("three_blocks", text(9000, 3), 8, comp=three_blocks(text(9000, 3))),
        Ent("text_70k", t70, 8),
        Ent("odd", b"x" * 13, 0),                       # shifts what follows off every alignment
        Ent("noise_100k_stored", noise(100 << 10, 9), 0),
        Ent("fixed", text(300, 4), 8, comp=raw_deflate(text(300, 4), 6, zlib.Z_FIXED)),
        Ent("stored_blocks", noise(70000, 5), 8, comp=raw_deflate(noise(70000, 5), 0)),
    ]


def lookalike_entries():
    ents = small_entries(40)
    fz = fake_header(0, 0, 0, 0)
    ents[2].cextra = struct.pack("<HH", 0x7777, len(fz)) + fz
    ents[5].fcomment = fz + fz
    ents[7] = Ent(b"n" + fake_header(0x41, 0x0120, 0x0120, 0x0120) + b"z", b"named like a header", 8)
    ents[9].fcomment = b"PK\x01\x02 short"
    ents[11].cextra = struct.pack("<HH", 0x7778, 50) + b"PK" + fz + b"\x01\x02"
    return ents


def nested_archive(comment: bytes = b"") -> bytes:
    inner = craft(small_entries(3), comment=b"inner")
    return craft(small_entries(2) + [Ent("inner.zip", inner, 0)], comment=comment)


def zipfile_written() -> bytes:
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as zf:
        zf.writestr("a.txt", text(5000, 11), zipfile.ZIP_DEFLATED)
        zf.writestr("dir/", b"")
        zf.writestr("dir/b.bin", noise(3000, 12), zipfile.ZIP_STORED)
        zf.writestr("dir/ümläut.txt", text(100, 13), zipfile.ZIP_DEFLATED)
        with zf.open(zipfile.ZipInfo("streamed64"), "w", force_zip64=True) as f:   # ZIP64 extra + data descriptor
            f.write(text(2000, 14))
        zf.writestr(zipfile.ZipInfo("empty"), b"")
        zf.comment = b"written by zipfile"
    return buf.getvalue()


COUNTS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name -> archive bytes; every one opens in zipfile"""
    c = {f"count_{n}": craft(small_entries(n)) for n in COUNTS}
    c["seams_600"] = craft(small_entries(600, 30))
    c["lookalikes"] = craft(lookalike_entries())
    c["nested_last"] = nested_archive()
    c["nested_last_comment"] = nested_archive(b"outer")   # the slow rule: the last PK\5\6 is the outer one
    c["payloads"] = craft(payload_entries())
    c["zip64_all"] = craft(payload_entries()[:6], zip64=True)
    mix = small_entries(9)
    mix[1].z64, mix[4].z64, mix[6].z64, mix[8].z64 = {"usize"}, {"csize", "off"}, {"off"}, {"usize", "csize", "off"}
    c["zip64_mix"] = craft(mix, tail64=True)
    c["comment_34"] = craft(small_entries(5), comment=b"c" * 34)
    c["prefix_70"] = craft(small_entries(5), prefix=b"#!/bin/sh\n" * 7)
    c["data_descriptors"] = craft(payload_entries()[:6], dd=True)
    c["local_extra"] = craft(small_entries(7), local_extra=struct.pack("<HH", 0x5455, 9) + b"\x01" + b"t" * 8)
    c["zip64_prefix_comment"] = craft(small_entries(4), zip64=True, prefix=b"PREF", comment=b"k" * 65535)
    c["zipfile_written"] = zipfile_written()
    return c


def comment_with_end_signature() -> bytes:
    """zipfile raises BadZipFile on this one: the last PK\\5\\6 lies inside the comment"""
    return craft(small_entries(3), comment=b"see PK\x05\x06 for details, and some more bytes behind it")


# ---- corrupt archives: (bytes, file status or 0, entry number or None, entry status) ----

def _eocd(z: bytes) -> int:
    return z.rfind(b"PK\x05\x06")


def _cdh(z: bytes, i: int) -> int:
    """the offset of central header i of a craft()ed archive without look-alikes"""
    p = struct.unpack_from("<I", z, _eocd(z) + 16)[0]
    for _ in range(i):
        n, m, k = struct.unpack_from("<HHH", z, p + 28)
        p += 46 + n + m + k
    return p


def _put(z: bytes, off: int, fmt: str, *v) -> bytes:
    b = bytearray(z)
    struct.pack_into(fmt, b, off, *v)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def corrupt_cases() -> dict:
    E = D.E
    base = craft(small_entries(6) + [Ent("st", b"stored bytes", 0)])
    e = _eocd(base)
    n = 7
    h3, h6 = _cdh(base, 3), _cdh(base, 6)
    lh3 = struct.unpack_from("<I", base, h3 + 42)[0]
    c = {
        "cut_end_record": (base[:-1], -E["E_ZHEAD"], None, 0),
        "no_end_record": (base[:e] + b"PK\x05\x07" + base[e + 4:], -E["E_ZHEAD"], None, 0),
        "tiny": (b"PK", -E["E_ZHEAD"], None, 0),
        "disk_number": (_put(base, e + 4, "<H", 1), -E["E_RANGE"], None, 0),
        "disk_counts": (_put(base, e + 8, "<H", n - 1), -E["E_RANGE"], None, 0),
        "one_too_many": (_put(base, e + 8, "<HH", n + 1, n + 1), -E["E_LEN"], None, 0),
        "one_too_few": (_put(base, e + 8, "<HH", n - 1, n - 1), -E["E_LEN"], None, 0),
        "cd_size_past_file": (_put(base, e + 12, "<I", len(base)), -E["E_RANGE"], None, 0),
        "method_12": (_put(base, h3 + 10, "<H", 12), 0, 3, -E["E_ZCMPMT"]),
        "encrypted": (_put(base, h3 + 8, "<H", 1), 0, 3, -E["E_RESERV"]),
        "local_signature": (_put(base, lh3, "<I", 0x04034B51), 0, 3, -E["E_ZHEAD"]),
        "csize_past_file": (_put(base, h3 + 20, "<I", len(base)), 0, 3, -E["E_RANGE"]),
        "stored_size_mismatch": (_put(base, h6 + 24, "<I", 13), 0, 6, -E["E_LEN"]),
    }
    return {"base": (base, 0, None, 0), **c}


def zipfile_entries(z: bytes):
    """[(ZipInfo, data offset or None, bytes)] as zipfile sees the archive"""
    f = io.BytesIO(z)
    out = []
    with zipfile.ZipFile(f) as zf:
        assert zf.testzip() is None
        for info in zf.infolist():
            with zf.open(info) as fh:
                pos = f.tell()   # ZipFile.open leaves the file right behind the local header
                data = fh.read()
            out.append((info, pos, data))
    return out


def entry_array(z: bytes):
    """(ZipStatus, numpy entries) of dmx_zip_index_host, whatever the status"""
    import ctypes
    L = D.lib()
    st = D.ZipStatus()
    buf = ctypes.create_string_buffer(z, len(z) or 1)
    assert L.dmx_zip_index_host(buf, len(z), None, 0, ctypes.byref(st)) == 0
    cap = st.nentries
    ent = np.zeros(max(cap, 1), dtype=D.ZipEntryDTYPE)
    assert L.dmx_zip_index_host(buf, len(z), ctypes.c_void_p(ent.ctypes.data), cap, ctypes.byref(st)) == 0
    return st, ent[:st.nentries]
