"""Reading any BGZF file, host side, no GPU: dmx_bgzf_index_max on files whose members hold up to
65 536 bytes (built with Python's zlib, tests/bgzf_read_inputs.py), its bound, the unchanged
32 KiB call, truncations of a 65 280-byte member, the walk under ASan / UBSan in a stand-alone
program, and the parts of dmx_bgzf_decode_host that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import deflate_compression_amd as D
from bgzf_read_inputs import EOF_MEMBER, HTS, TOP, bgzf_file, entries, hts_sizes, want_entries

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 32768, 32769, HTS, TOP]


def _text(n: int, seed: int = 21) -> bytes:
    return D.gen_text(max(n, 1), seed).tobytes()[:n]


def _index_max(z: bytes, bound: int, cap=None):
    """the C call itself: (status, entries, crcs, nblk, total)"""
    L = D.lib()
    buf = (ctypes.c_uint8 * max(len(z), 1)).from_buffer_copy(z or b"\0")
    nb, tot = ctypes.c_uint32(77), ctypes.c_uint64(77)
    n = 64 if cap is None else cap
    idx, crc = np.zeros(24 * max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32)
    r = L.dmx_bgzf_index_max(ctypes.cast(buf, ctypes.c_void_p), len(z), bound, ctypes.c_void_p(idx.ctypes.data),
                             ctypes.c_void_p(crc.ctypes.data), n, ctypes.byref(nb), ctypes.byref(tot))
    k = min(nb.value, n)
    return r, entries(idx[:24 * k]), crc[:k].tolist(), nb.value, tot.value


def _code(z: bytes, bound: int) -> int:
    try:
        D.bgzf_index(z, bound)
    except D.DeflateError as e:
        return e.code
    return 0


@pytest.fixture(scope="module")
def five():
    data = _text(sum(SIZES))
    z, lay = bgzf_file(data, SIZES, 6)
    return data, z, lay


def test_index_max_members_up_to_65536(five):
    import zlib
    data, z, lay = five
    r, ent, crcs, nb, tot = _index_max(z, D.DMX_BGZF_MAX_ISIZE)
    assert r == 0 and nb == len(SIZES) and tot == len(data)
    assert ent == want_entries(lay)
    assert crcs == [zlib.crc32(data[o:o + n]) for _, _, o, n in lay]
    idx, c2, total = D.bgzf_index(z, 65536)
    assert entries(idx) == ent and c2.tolist() == crcs and total == len(data)
    # cap too small: -E_SZ, the needed count and the total still reported
    r, ent1, _, nb, tot = _index_max(z, 65536, cap=2)
    assert r == -D.E["E_SZ"] and nb == len(SIZES) and tot == len(data) and ent1 == ent[:2]
    # an empty member in the middle and the end-of-file member give no entry
    z2, lay2 = bgzf_file(data[:70000], [1234, 0, 65280, 3486], 1)
    assert _index_max(z2, 65536)[1] == want_entries(lay2) and len(want_entries(lay2)) == 3


def test_index_max_bound(five):
    _, z, _ = five
    RANGE = -D.E["E_RANGE"]
    for bound, want in ((65279, RANGE), (65280, RANGE), (65535, RANGE), (65536, 0)):
        assert _index_max(z, bound)[0] == want, bound
        assert _code(z, bound) == want, bound
    zh, _ = bgzf_file(_text(3 * HTS + 17, 22), hts_sizes(3 * HTS + 17), 6)   # the largest member: 65 280
    for bound, want in ((32768, RANGE), (65279, RANGE), (65280, 0), (65536, 0)):
        assert _index_max(zh, bound)[0] == want, bound
    # the bound itself: 1..65536, whatever the file; nothing is reported
    for z0 in (z, zh, EOF_MEMBER, b""):
        for bound in (0, 65537, 1 << 31, 0xFFFFFFFF):
            r, _, _, nb, tot = _index_max(z0, bound)
            assert r == RANGE and nb == 0 and tot == 0, bound
    assert _index_max(EOF_MEMBER, 1)[0] == 0 and _index_max(b"", 1)[0] == 0
    zs, _ = bgzf_file(b"ab", [1, 1], 6)
    assert _index_max(zs, 1)[0] == 0


def test_index_32k_call_unchanged(five):
    _, z, _ = five
    L = D.lib()
    RANGE = -D.E["E_RANGE"]

    def old(zz, cap=64):
        buf = (ctypes.c_uint8 * len(zz)).from_buffer_copy(zz)
        nb, tot = ctypes.c_uint32(0), ctypes.c_uint64(0)
        idx, crc = np.zeros(24 * cap, np.uint8), np.zeros(cap, np.uint32)
        r = L.dmx_bgzf_index(ctypes.cast(buf, ctypes.c_void_p), len(zz), ctypes.c_void_p(idx.ctypes.data),
                             ctypes.c_void_p(crc.ctypes.data), cap, ctypes.byref(nb), ctypes.byref(tot))
        k = min(nb.value, cap)
        return r, entries(idx[:24 * k]), crc[:k].tolist(), nb.value, tot.value

    assert old(z)[0] == RANGE and _code(z, 32768) == RANGE
    with pytest.raises(D.DeflateError) as ei:
        D.bgzf_index(z)   # the default bound is the old one
    assert ei.value.code == RANGE
    data = _text(100000, 23)
    small, lay = bgzf_file(data, [32768, 1, 0, 32767, 20000, 14464], 6)
    got = old(small)
    assert got[0] == 0 and got == _index_max(small, 32768) and got[1] == want_entries(lay)
    a, b = D.bgzf_index(small), D.bgzf_index(small, 32768)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[2] == b[2] == len(data)


@pytest.mark.parametrize("level", [0, 6])
def test_truncations_of_a_65280_member(level):
    """what the walk gives for a cut file does not depend on the member's size: -E_LEN inside a
    member, 0 at a member boundary (level 0: a stored member of 65 316 bytes, sampled; level 6:
    every truncation)"""
    data = _text(HTS + 100, 24)
    z, lay = bgzf_file(data, [HTS, 100], level, eof=False)
    m0 = lay[0][1]
    cuts = range(1, len(z)) if level else sorted(set(list(range(1, 64)) + list(range(1, len(z), 997)) +
                                                      list(range(m0 - 64, m0 + 64)) + list(range(len(z) - 64, len(z)))))
    LEN = -D.E["E_LEN"]
    for t in cuts:
        r, ent, _, nb, tot = _index_max(z[:t], 65536)
        assert r == (0 if t == m0 else LEN), t
        if t == m0:
            assert ent == [(8 * 18, 0, HTS)] and tot == HTS
    assert _index_max(z, 65536)[0] == 0 and _index_max(b"", 65536)[0] == 0


def test_bgzf_index_max_asan_ubsan(tmp_path):
    """tests/c/bgzf_max_asan.c: dmx_bgzf_index_max compiled with AddressSanitizer + UBSan in a
    stand-alone program, on valid files with 64 KiB members, on exact-size copies of their
    truncations and on bit flips of every header and trailer: 0 or -E_*, no sanitizer finding."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.bgzf_max"])
    n = 3 * HTS + 17
    files = []
    for k, (data, sizes, level) in enumerate(((_text(n, 25), hts_sizes(n), 6),
                                              (_text(sum(SIZES), 26), SIZES, 1),
                                              (_text(HTS + 5, 27), [HTS, 0, 5], 0),
                                              (bytes(TOP) + b"x", [TOP, 1], 9))):
        f = tmp_path / f"f{k}.bgzf"
        f.write_bytes(bgzf_file(data, sizes, level)[0])
        files.append(str(f))
    p = subprocess.run([os.path.join(REPO, "build", "c", "bgzf_max_asan")] + files, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "0 failed checks" in p.stdout


def test_decode_host_without_a_device():
    """dmx_bgzf_decode_host answers from the index alone where nothing is to decode: an empty
    file and one of empty members give 0 bytes, a capacity that is too small the decoded length
    and -E_SZ, a file that does not index the walk's status"""
    assert D.decompress_bgzf(b"") == b"" and D.decompress_bgzf(EOF_MEMBER) == b""
    assert D.decompress_bgzf(EOF_MEMBER + EOF_MEMBER, verify=False) == b""
    L = D.lib()
    z, _ = bgzf_file(_text(HTS + 7, 28), [HTS, 7], 6)
    buf = (ctypes.c_uint8 * len(z)).from_buffer_copy(z)
    out = (ctypes.c_uint8 * (HTS + 6))()
    olen = ctypes.c_uint64(0)
    r = L.dmx_bgzf_decode_host(ctypes.cast(buf, ctypes.c_void_p), len(z), ctypes.cast(out, ctypes.c_void_p), HTS + 6,
                               ctypes.byref(olen), 1)
    assert r == -D.E["E_SZ"] and olen.value == HTS + 7 and bytes(out) == bytes(HTS + 6)
    r = L.dmx_bgzf_decode_host(ctypes.cast(buf, ctypes.c_void_p), len(z) - 1, None, 0, ctypes.byref(olen), 1)
    assert r == -D.E["E_LEN"] and olen.value == 0
    with pytest.raises(D.DeflateError) as ei:
        D.decompress_bgzf(z[:-30])
    assert ei.value.code == -D.E["E_LEN"]
    assert L.dmx_bgzf_decode_host(None, 0, None, 0, None, 1) == -D.E["E_INVAL"]
