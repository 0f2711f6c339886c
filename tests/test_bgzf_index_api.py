"""The device BGZF index without a device: the exports and their declarations, the argument errors
that dmx_bgzf_index_async and dmx_bgzf_decode_device return before any device call, the size of the
work buffer, and the host twin of the kernels (tests/c/bgzf_dindex_model.cpp: the stages as loops
over the text the kernel threads run) against dmx_bgzf_index_max under ASan + UBSan."""
import ctypes
import os
import subprocess

import deflate_compression_amd as D
from bgzf_read_inputs import HTS, TOP, bgzf_file

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE = -E["E_INVAL"], -E["E_RANGE"]
EXPORTS = ("dmx_bgzf_index_work", "dmx_bgzf_index_geometry", "dmx_bgzf_index_async", "dmx_bgzf_decode_device")


def _text(n: int, seed: int) -> bytes:
    return D.gen_text(max(n, 1), seed).tobytes()[:n]


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in EXPORTS:
        f = getattr(L, name)
        assert f.argtypes is not None, name   # a signature is set
        assert name + "(" in hdr, name
    assert "dmx_bgzf_index_status" in hdr
    for name in ("bgzf_index_gpu", "inflate_bgzf_tensor"):
        assert name in D.__all__ and callable(getattr(D, name))


def _index(z=0x1000, zbytes=64, max_isize=65536, index=0x2000, crc=0x3000, cap=4, work=0x4000, work_bytes=None,
           status=0x5000):
    """dmx_bgzf_index_async on made-up addresses: an argument error returns before they are used"""
    L = D.lib()
    if work_bytes is None:
        work_bytes = L.dmx_bgzf_index_work(min(zbytes, 1 << 20), 16)
    vp = ctypes.c_void_p
    return L.dmx_bgzf_index_async(vp(z), zbytes, max_isize, vp(index), vp(crc), cap, vp(work), work_bytes, vp(status), vp(0))


def test_index_argument_errors():
    L = D.lib()
    need = L.dmx_bgzf_index_work(64, 1)
    assert _index(z=0) == INVAL                       # no file, but bytes
    assert _index(status=0) == INVAL
    assert _index(index=0, cap=1) == INVAL
    assert _index(index=0x2004) == INVAL              # 8-byte alignment of the entries
    assert _index(crc=0x3002) == INVAL                # 4-byte alignment of the CRC words
    assert _index(work=0x4080) == INVAL               # 256-byte alignment of the work buffer
    assert _index(work=0) == INVAL
    assert _index(work_bytes=need - 1) == INVAL
    assert _index(work_bytes=0) == INVAL
    for bad in (0, 65537, 0xFFFFFFFF):
        assert _index(max_isize=bad) == RANGE
    assert _index(zbytes=0xFFFFFFF1, work_bytes=1 << 40) == RANGE
    assert _index(zbytes=1 << 40, work_bytes=1 << 50) == RANGE


def test_decode_argument_errors():
    L = D.lib()
    vp = ctypes.c_void_p
    olen = ctypes.c_uint64(77)
    assert L.dmx_bgzf_decode_device(vp(0), 64, vp(0x2000), 64, ctypes.byref(olen), 1, vp(0)) == INVAL
    assert L.dmx_bgzf_decode_device(vp(0x1000), 64, vp(0x2000), 64, None, 1, vp(0)) == INVAL
    assert L.dmx_bgzf_decode_device(vp(0x1000), 64, vp(0), 64, ctypes.byref(olen), 1, vp(0)) == INVAL
    assert L.dmx_bgzf_decode_device(vp(0x1000), 0xFFFFFFF1, vp(0x2000), 64, ctypes.byref(olen), 1, vp(0)) == RANGE
    assert olen.value == 0
    # an empty file decodes to nothing, and needs no device for it
    olen.value = 77
    assert L.dmx_bgzf_decode_device(vp(0), 0, vp(0), 0, ctypes.byref(olen), 1, vp(0)) == 0 and olen.value == 0


def test_work_size_and_geometry():
    L = D.lib()
    for zbytes in (0, 1, 28, 65536, 100 << 20, 0xFFFFFFF0):
        last = 0
        for m in (0, 1, 2, 4, 15, 16, 17, 1000, 1 << 20, 0xFFFFFFFF):
            w = L.dmx_bgzf_index_work(zbytes, m)
            assert w > 0 and w % 256 == 0 and w >= last, (zbytes, m, w)
            last = w
    assert L.dmx_bgzf_index_work(1 << 20, 4096) <= L.dmx_bgzf_index_work(1 << 21, 4096)
    tile = ctypes.c_uint32(0)
    L.dmx_bgzf_index_geometry(ctypes.byref(tile))
    assert tile.value >= 16 and tile.value & (tile.value - 1) == 0


def nested_file():
    """a stored member whose data is a whole three-member BGZF file with its end-of-file member"""
    inner, _ = bgzf_file(_text(3000, 41), [1000, 1500, 500], 6)
    return bgzf_file(inner, [len(inner)], 0)[0], inner


def test_host_twin_asan_ubsan(tmp_path):
    """tests/c/bgzf_dindex_model.cpp prints `0 failed checks`: on each file, on every truncation of
    it and on every single-bit flip of its members' headers and trailers the stages of the device
    index, run as loops, give dmx_bgzf_index_max's status, count, total, entries and CRC words."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.bgzf_dindex"])
    five = [1, 32768, 32769, HTS, TOP]
    inputs = (bgzf_file(_text(HTS + 5, 42), [HTS, 0, 5], 0)[0],
              bgzf_file(_text(sum(five), 43), five, 1)[0],
              nested_file()[0],
              bgzf_file(_text(300, 44), [1] * 300, 6)[0])
    files = []
    for k, z in enumerate(inputs):
        f = tmp_path / f"f{k}.bgzf"
        f.write_bytes(z)
        files.append(str(f))
    exe = os.path.join(REPO, "build", "c", "bgzf_dindex_model")
    runs = [subprocess.Popen([exe, f], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for f in files]   # side by side
    for f, p in zip(files, runs):
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, f + ": " + out[-2000:] + err[-4000:]
        assert "0 failed checks" in out, f
