"""The batched BGZF range reads without a device: the exports and their declarations, the argument
errors that dmx_bgzf_read_ranges_async and dmx_bgzf_read_device return before any device call, the
size of the work buffer, the two structs, and the host twin of the kernels
(tests/c/bgzf_ranges_model.cpp: the planning stages and the gather as loops over the text the
kernel threads run, scan tiles shrunk to 4 and 8) against brute force under ASan + UBSan."""
import ctypes
import os
import subprocess

import pytest

import deflate_compression_amd as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE = -E["E_INVAL"], -E["E_RANGE"]
EXPORTS = ("dmx_bgzf_ranges_work", "dmx_bgzf_ranges_geometry", "dmx_bgzf_read_ranges_async", "dmx_bgzf_read_device")
vp = ctypes.c_void_p


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in EXPORTS:
        f = getattr(L, name)
        assert f.argtypes is not None, name   # a signature is set
        assert name + "(" in hdr, name
    for name in ("dmx_brange", "dmx_bgzf_ranges_status", "DMX_RANGES_VIRTUAL 1u"):
        assert name in hdr, name
    for name in ("bgzf_read_ranges", "bgzf_pread", "bgzf_voffset", "DMX_RANGES_VIRTUAL"):
        assert name in D.__all__ and hasattr(D, name), name
    assert D.DMX_RANGES_VIRTUAL == 1
    assert D.bgzf_voffset(0x1234, 0x56) == 0x12340056
    assert D.bgzf_voffset((1 << 48) - 1, 65535) == (1 << 64) - 1
    for bad in ((0, 65536), (1 << 48, 0), (-1, 0), (0, -1)):
        with pytest.raises(ValueError):
            D.bgzf_voffset(*bad)


def test_struct_sizes():
    assert ctypes.sizeof(D.BRange) == 16
    assert ctypes.sizeof(D.RangesStatus) == 32
    assert (D.RangesStatus.status.offset, D.RangesStatus.nmembers.offset, D.RangesStatus.out_len.offset,
            D.RangesStatus.scratch_len.offset, D.RangesStatus.bad.offset, D.RangesStatus.reserved.offset) == (0, 4, 8, 16, 24, 28)
    assert (D.BRange.off.offset, D.BRange.len.offset) == (0, 8)


def _ranges(z=0x1000, zbytes=64, index=0x2000, crc=0x3000, nblk=4, ranges=0x4000, nranges=3, flags=0, out=0x5000, out_cap=64,
            out_off=0x6000, max_members=4, scratch_bytes=1 << 18, work=0x10000, work_bytes=None, status=0x7000):
    """dmx_bgzf_read_ranges_async on made-up addresses: an argument error returns before they are used"""
    L = D.lib()
    if work_bytes is None:
        work_bytes = L.dmx_bgzf_ranges_work(nblk, min(nranges, 1 << 20), max_members, scratch_bytes)
    return L.dmx_bgzf_read_ranges_async(vp(z), zbytes, vp(index), vp(crc), nblk, vp(ranges), nranges, flags, vp(out), out_cap,
                                        vp(out_off), max_members, scratch_bytes, vp(work), work_bytes, vp(status), vp(0))


def test_async_argument_errors():
    L = D.lib()
    need = L.dmx_bgzf_ranges_work(4, 3, 4, 1 << 18)
    assert _ranges(z=0) == INVAL                       # no file, but bytes
    assert _ranges(status=0) == INVAL
    assert _ranges(work=0) == INVAL
    assert _ranges(out_off=0) == INVAL
    assert _ranges(index=0) == INVAL                   # NULL with nblk > 0
    assert _ranges(ranges=0) == INVAL                  # NULL with nranges > 0
    assert _ranges(out=0) == INVAL                     # NULL with out_cap > 0
    assert _ranges(index=0x2004) == INVAL              # 8-byte alignment of the entries
    assert _ranges(ranges=0x4004) == INVAL             # ... of the ranges
    assert _ranges(out_off=0x6004) == INVAL            # ... of the offsets
    assert _ranges(status=0x7004) == INVAL             # ... of the record
    assert _ranges(crc=0x3002) == INVAL                # 4-byte alignment of the CRC words
    assert _ranges(work=0x10080) == INVAL              # 256-byte alignment of the work buffer
    assert _ranges(work_bytes=need - 1) == INVAL
    assert _ranges(work_bytes=0) == INVAL
    assert _ranges(zbytes=0xFFFFFFF1) == RANGE
    assert _ranges(zbytes=1 << 40) == RANGE
    assert _ranges(nranges=0x80000000, work_bytes=1 << 60) == RANGE
    assert _ranges(nranges=0xFFFFFFFF, work_bytes=1 << 60) == RANGE
    for flags in (2, 3, 0x80000000):
        assert _ranges(flags=flags) == RANGE


def _device(z=0x1000, zbytes=64, index=0x2000, crc=0x3000, nblk=4, ranges=0x4000, nranges=3, flags=0, out=0x5000, out_cap=64,
            out_off=0x6000, olen=True, verify=1):
    L = D.lib()
    n = ctypes.c_uint64(77)
    r = L.dmx_bgzf_read_device(vp(z), zbytes, vp(index), vp(crc), nblk, vp(ranges), nranges, flags, vp(out), out_cap, vp(out_off),
                               ctypes.byref(n) if olen else None, verify, vp(0))
    return r, n.value


def test_device_argument_errors():
    assert _device(olen=False)[0] == INVAL
    for kw in (dict(z=0), dict(index=0), dict(ranges=0), dict(out=0), dict(out_off=0), dict(crc=0, verify=1)):
        assert _device(**kw)[0] == INVAL, kw
    for kw in (dict(index=0x2004), dict(ranges=0x4004), dict(out_off=0x6004), dict(crc=0x3002)):
        assert _device(**kw) == (INVAL, 0), kw
    for kw in (dict(zbytes=0xFFFFFFF1), dict(nranges=0x80000000), dict(flags=2)):
        assert _device(**kw) == (RANGE, 0), kw


def test_work_size_and_geometry():
    L = D.lib()
    grid = (0, 1, 2, 255, 256, 257, 4096, 1 << 20, 0xFFFFFFFF)
    base = (3052, 4096, 1000, 1 << 26)
    for arg in range(4):
        last = 0
        for v in grid + ((1 << 40, (1 << 64) - 1) if arg == 3 else ()):
            a = list(base)
            a[arg] = v
            w = L.dmx_bgzf_ranges_work(*a)
            assert w > 0 and w % 256 == 0 and w >= last, (arg, v, w)
            last = w
    assert L.dmx_bgzf_ranges_work(0, 0, 0, 0) >= 256
    # the decode's tables (8 KiB per slot) and the scratch are in it
    assert L.dmx_bgzf_ranges_work(10, 10, 100, 0) - L.dmx_bgzf_ranges_work(10, 10, 0, 0) >= 100 * 8192
    assert L.dmx_bgzf_ranges_work(10, 10, 0, 1 << 20) - L.dmx_bgzf_ranges_work(10, 10, 0, 0) >= 1 << 20
    t, r = D.ranges_geometry()
    assert t >= 64 and t & (t - 1) == 0 and r >= 64 and r & (r - 1) == 0


def test_host_twin_asan_ubsan():
    """tests/c/bgzf_ranges_model.cpp ends with `0 failed checks`: for every (off, len) and every
    virtual offset of small layouts with empty members, for broken indexes and for seeded random
    batches, the stages of the range read, run as loops with scan tiles of 4 members and 8 ranges,
    give brute force's record, offsets, sub-index and bytes, and leave d_out alone when they must."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.bgzf_ranges"])
    exe = os.path.join(REPO, "build", "c", "bgzf_ranges_model")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert " checks, 0 failed checks" in p.stdout
