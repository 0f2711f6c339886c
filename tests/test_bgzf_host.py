"""BGZF container (DMX_F_BGZF), host side, no GPU: dmx_bgzf_index on files assembled from the
oracle's DEFLATE data in the shape the encoder writes (18-byte header with BSIZE, data, CRC-32 /
ISIZE, the 28-byte end-of-file member), its error codes and every truncation; the output
bound; DMX_FORMAT validation; the shard flags; the index walk under ASan / UBSan."""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_compression_amd as D
from deflate_compression_amd import shard
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR16 = bytes([0x1F, 0x8B, 0x08, 0x04, 0, 0, 0, 0, 0, 0xFF, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00])
EOF_MEMBER = HDR16 + bytes([0x1B, 0x00, 0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0])


def member(deflate: bytes, block: bytes, extra_before: bytes = b"", extra_after: bytes = b"") -> bytes:
    """A BGZF member around `deflate`; extra_*: other FEXTRA subfields around "BC"."""
    xlen = 6 + len(extra_before) + len(extra_after)
    size = 12 + xlen + len(deflate) + 8
    return (HDR16[:10] + struct.pack("<H", xlen) + extra_before + b"BC\x02\x00" + struct.pack("<H", size - 1) +
            extra_after + deflate + struct.pack("<II", zlib.crc32(block), len(block)))


def assemble(data: bytes, sw: int, **kw) -> bytes:
    out = []
    for o in range(0, len(data), sw):
        blk = data[o:o + sw]
        out.append(member(O.compress(blk, sw=sw, **kw)[2:-4], blk))
    return b"".join(out) + EOF_MEMBER


def entries(idx: np.ndarray):
    """[(bit, out_off, out_len)] of a dmx_iblock array"""
    a = idx.view(np.uint64).reshape(-1, 3)
    return [(int(r[0]), int(r[1]), int(r[2] & 0xFFFFFFFF)) for r in a]


def _data(n: int) -> bytes:
    t = D.gen_text(max(n, 1), 11).tobytes()[:n]
    r = D.gen_random(max(n, 1), 12).tobytes()[:n]
    return t[:n // 2] + r[n // 2:]   # text, then stored blocks


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("sw", [32768, 4097, 1000])
def test_index_of_oracle_files(sw, fast):
    kw = dict(max_chain=7, lazy=True, deep=True, store_check=True) if fast else {}
    for n in (0, 1, sw - 1, sw, sw + 1, 3 * sw + 17):
        data = _data(n)
        z = assemble(data, sw, **kw)
        assert gzip.decompress(z) == data, (sw, n)
        idx, crcs, total = D.bgzf_index(z)
        nblk = (n + sw - 1) // sw
        assert total == n and crcs.size == nblk and idx.size == 24 * nblk
        want, off = [], 0
        for b in range(nblk):
            blk = data[b * sw:(b + 1) * sw]
            size = 18 + len(O.compress(blk, sw=sw, **kw)) - 6 + 8
            want.append((8 * (off + 18), b * sw, len(blk)))
            assert crcs[b] == zlib.crc32(blk)
            off += size
        assert entries(idx) == want, (sw, n)
        assert off + 28 == len(z)


def test_index_skips_empty_members_and_reads_other_subfields():
    a, b = b"first member " * 40, b"second"
    da, db = O.compress(a)[2:-4], O.compress(b)[2:-4]
    xa = b"XY\x03\x00abc"           # a subfield before BC
    xb = b"ZZ\x00\x00"              # an empty one behind it
    z = member(da, a, extra_before=xa) + EOF_MEMBER + member(db, b, extra_after=xb) + EOF_MEMBER
    assert gzip.decompress(z) == a + b
    idx, crcs, total = D.bgzf_index(z)
    m0 = len(member(da, a, extra_before=xa))
    assert entries(idx) == [(8 * (18 + len(xa)), 0, len(a)), (8 * (m0 + 28 + 18 + len(xb)), len(a), len(b))]
    assert list(crcs) == [zlib.crc32(a), zlib.crc32(b)] and total == len(a) + len(b)
    assert D.bgzf_index(b"")[2] == 0 and D.bgzf_index(EOF_MEMBER)[1].size == 0


def _code(z: bytes) -> int:
    try:
        D.bgzf_index(z)
    except D.DeflateError as e:
        return e.code
    return 0


def test_index_error_codes():
    a, b = b"abcabcabc" * 100, bytes(range(256)) * 4
    ma, mb = member(O.compress(a)[2:-4], a), member(O.compress(b)[2:-4], b)
    z = ma + mb
    assert _code(z) == 0 and _code(ma) == 0
    # every truncation of the 2-member file: -E_LEN, except at a member boundary
    for t in range(1, len(z)):
        assert _code(z[:t]) == (0 if t == len(ma) else -D.E["E_LEN"]), t
    # not gzip / not deflate / no FEXTRA / no BC subfield / BC with another length
    for k, v in ((0, 0x1E), (1, 0x8A), (2, 7), (3, 0), (12, ord("X")), (14, 3)):
        bad = bytearray(z)
        bad[len(ma) + k] = v
        assert _code(bytes(bad)) == -D.E["E_ZHEAD"], k
    zlib_stream = zlib.compress(a)
    assert _code(zlib_stream + bytes(20)) == -D.E["E_ZHEAD"]
    assert _code(gzip.compress(a)) == -D.E["E_ZHEAD"]          # a plain gzip member: no FEXTRA
    # BSIZE too small for header + trailer
    tiny = bytearray(ma)
    tiny[16:18] = struct.pack("<H", 20)
    assert _code(bytes(tiny)) == -D.E["E_ZHEAD"]
    # ISIZE past the GPU decoder's 32 KiB window (htslib's default 65280-byte blocks)
    big = bytes(40000)
    c = zlib.compressobj(6, wbits=-15)
    assert _code(member(c.compress(big) + c.flush(), big) + EOF_MEMBER) == -D.E["E_RANGE"]
    # cap too small: -E_SZ, the needed count still reported
    L = D.lib()
    import ctypes
    buf = (ctypes.c_uint8 * len(z)).from_buffer_copy(z)
    one = np.zeros(24, np.uint8)
    nb, tot = ctypes.c_uint32(0), ctypes.c_uint64(0)
    r = L.dmx_bgzf_index(ctypes.cast(buf, ctypes.c_void_p), len(z), ctypes.c_void_p(one.ctypes.data), None, 1,
                         ctypes.byref(nb), ctypes.byref(tot))
    assert r == -D.E["E_SZ"] and nb.value == 2 and tot.value == len(a) + len(b)
    assert entries(one) == [(8 * 18, 0, len(a))]


def test_max_compressed_bgzf():
    for sw in (32768, 4097, 1000):
        for n in (0, 1, sw - 1, sw, sw + 1, 3 * sw + 17, 1 << 30):
            nblk = (n + sw - 1) // sw
            for flags in (D.DMX_BGZF, D.DMX_F_BGZF, D.DMX_BGZF | D.DMX_GZIP):
                assert D.max_compressed(n, sw, flags) == D.max_compressed(n, sw) + 26 * nblk + 28, (sw, n)
    assert D.DMX_F_BGZF == 1024 and D.DMX_BGZF == D.DMX_F_BGZF | D.DMX_F_FINAL


def test_shard_flags_bgzf():
    assert [shard.shard_flags_bgzf(r, 3) for r in range(3)] == [D.DMX_F_BGZF, D.DMX_F_BGZF, D.DMX_BGZF]
    assert shard.shard_flags_bgzf(0, 1) == D.DMX_BGZF


@pytest.mark.parametrize("env", [{"DMX_FORMAT": "bgzf", "DMX_DICT": "1"}, {"DMX_FORMAT": "bgzf", "DMX_SPLIT": "1"},
                                 {"DMX_FORMAT": "bogus"}, {"DMX_FORMAT": "BGZF"}])
def test_bad_format_combinations_fail_before_encoding(tmp_path, monkeypatch, env):
    """DMX_FORMAT=bgzf with DMX_DICT / DMX_SPLIT, and unknown values, are -E_INVAL before
    anything is read, encoded or written (no GPU needed: the check comes first)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
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


def test_bgzf_index_asan_ubsan(tmp_path):
    """tests/c/bgzf_asan.c: dmx_bgzf_index compiled with AddressSanitizer + UBSan in a
    stand-alone program, on valid files, on exact-size copies of every truncation and on bit
    flips of the headers and trailers: 0 or -E_*, no sanitizer finding."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.bgzf"])
    files = []
    for k, (sw, n) in enumerate(((32768, 3 * 32768 + 17), (1000, 2500), (4097, 1))):
        f = tmp_path / f"f{k}.bgzf"
        f.write_bytes(assemble(_data(n), sw))
        files.append(str(f))
    p = subprocess.run([os.path.join(REPO, "build", "c", "bgzf_asan")] + files, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "0 failed checks" in p.stdout
