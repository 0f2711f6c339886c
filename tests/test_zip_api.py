"""ZIP archives without a device: the exports and their declarations, the argument errors that
dmx_zip_index_async and dmx_zip_read_async return before any device call, the sizes of the work
buffers, dmx_zip_index_host against CPython's zipfile on every archive of zip_inputs.cases(), the
statuses of corrupt archives, and the host twin of the device index (tests/c/zip_model.cpp: the
stages as loops over the text the kernel threads run) against the host walk under ASan + UBSan."""
import ctypes
import io
import os
import subprocess
import zipfile

import numpy as np
import pytest

import deflate_compression_amd as D
import zip_inputs as Z

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE = -E["E_INVAL"], -E["E_RANGE"]
EXPORTS = ("dmx_zip_index_host", "dmx_zip_index_work", "dmx_zip_index_async", "dmx_zip_read_work", "dmx_zip_read_async",
           "dmx_zip_index_geometry", "dmx_zip_read_geometry")


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in EXPORTS:
        f = getattr(L, name)
        assert f.argtypes is not None, name
        assert name + "(" in hdr, name
    for name in ("dmx_zip_status", "dmx_zip_entry", "DMX_ZIP_VERIFY"):
        assert name in hdr
    for name in ("ZipEntryDTYPE", "ZipStatus", "ZipIndex", "zip_index", "zip_index_gpu", "zip_index_async",
                 "zip_read_async", "zip_read", "unzip"):
        assert name in D.__all__ and getattr(D, name) is not None
    assert ctypes.sizeof(D.ZipStatus) == 40 and np.dtype(D.ZipEntryDTYPE).itemsize == 64


def _index(z=0x1000, zbytes=64, entries=0x2000, cap=4, work=0x4000, work_bytes=None, status=0x5000):
    """dmx_zip_index_async on made-up addresses: an argument error returns before they are used"""
    L = D.lib()
    if work_bytes is None:
        work_bytes = L.dmx_zip_index_work(min(zbytes, 1 << 20), 16)
    vp = ctypes.c_void_p
    return L.dmx_zip_index_async(vp(z), zbytes, vp(entries), cap, vp(work), work_bytes, vp(status), vp(0))


def test_index_argument_errors():
    L = D.lib()
    need = L.dmx_zip_index_work(64, 1)
    assert _index(z=0) == INVAL
    assert _index(status=0) == INVAL
    assert _index(entries=0, cap=1) == INVAL
    assert _index(entries=0x2004) == INVAL
    assert _index(status=0x5004) == INVAL
    assert _index(work=0x4080) == INVAL
    assert _index(work=0) == INVAL
    assert _index(work_bytes=need - 1) == INVAL
    assert _index(work_bytes=0) == INVAL
    assert _index(zbytes=0xFFFFFFF1, work_bytes=1 << 40) == RANGE
    assert _index(zbytes=1 << 40, work_bytes=1 << 50) == RANGE


def _read(z=0x1000, zbytes=64, entries=0x2000, nentries=4, sel=0x3000, nsel=4, flags=1, out=0x6000, out_bytes=64,
          offsets=0x7000, results=0x8000, work=0x4000, work_bytes=None, status=0x5000):
    L = D.lib()
    if work_bytes is None:
        work_bytes = L.dmx_zip_read_work(nsel)
    vp = ctypes.c_void_p
    return L.dmx_zip_read_async(vp(z), zbytes, vp(entries), nentries, vp(sel), nsel, flags, vp(out), out_bytes, vp(offsets),
                                vp(results), vp(work), work_bytes, vp(status), vp(0))


def test_read_argument_errors():
    L = D.lib()
    assert _read(z=0) == INVAL
    assert _read(entries=0) == INVAL
    assert _read(out=0) == INVAL
    assert _read(offsets=0) == INVAL
    assert _read(results=0) == INVAL
    assert _read(status=0) == INVAL
    assert _read(work=0) == INVAL
    assert _read(sel=0, nsel=3) == INVAL                 # no selectors means all entries
    assert _read(entries=0x2004) == INVAL
    assert _read(offsets=0x7004) == INVAL
    assert _read(results=0x8004) == INVAL
    assert _read(status=0x5004) == INVAL
    assert _read(sel=0x3002) == INVAL
    assert _read(work=0x4080) == INVAL
    assert _read(work_bytes=L.dmx_zip_read_work(4) - 1) == INVAL
    assert _read(flags=2) == RANGE
    assert _read(flags=16) == RANGE                      # DMX_BATCH_MEASURE has no meaning here
    assert _read(zbytes=0xFFFFFFF1) == RANGE


def test_work_sizes():
    L = D.lib()
    for zbytes in (0, 1, 22, 65536, 100 << 20, 0xFFFFFFF0):
        last = 0
        for m in (0, 1, 2, 15, 16, 17, 1000, 1 << 20, 0xFFFFFFFF):
            w = L.dmx_zip_index_work(zbytes, m)
            assert w > 0 and w % 256 == 0 and w >= last, (zbytes, m, w)
            last = w
    assert L.dmx_zip_index_work(1 << 20, 4096) <= L.dmx_zip_index_work(1 << 21, 4096)
    last = 0
    for n in (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 1 << 20, 0xFFFFFFFF):
        w = L.dmx_zip_read_work(n)
        assert w > 0 and w % 256 == 0 and w >= last and w >= L.dmx_inflate_batch_work(n), (n, w)
        last = w
    tile, span = ctypes.c_uint32(0), ctypes.c_uint32(0)
    L.dmx_zip_index_geometry(ctypes.byref(tile))
    L.dmx_zip_read_geometry(ctypes.byref(span))
    assert tile.value >= 16 and tile.value & (tile.value - 1) == 0
    assert span.value >= 16 and span.value % 16 == 0


@pytest.mark.parametrize("name", sorted(Z.cases()))
def test_host_index_matches_zipfile(name):
    z = Z.cases()[name]
    ref = Z.zipfile_entries(z)
    ix = D.zip_index(z)
    assert ix.status.status == 0 and len(ix) == len(ref) == ix.status.nentries
    run = 0
    for e, (info, pos, data) in zip(ix.host, ref):
        assert int(e["status"]) == 0, info.filename
        assert (int(e["method"]), int(e["flags"])) == (info.compress_type, info.flag_bits)
        assert (int(e["csize"]), int(e["usize"]), int(e["crc"])) == (info.compress_size, info.file_size, info.CRC)
        assert int(e["hdr_off"]) == info.header_offset        # zipfile has added concat
        assert int(e["data_off"]) == pos, info.filename
        assert int(e["out_off"]) == run
        run += info.file_size
        # the bytes at data_off are the entry
        comp = z[pos:pos + info.compress_size]
        assert (comp if info.compress_type == 0 else __import__("zlib").decompress(comp, -15)) == data
    assert ix.out_len == run
    assert ix.names == [info.orig_filename for info, _, _ in ref]
    if ref:
        last = ref[-1][0].orig_filename
        assert ix.names[ix.find(last)] == last
    with pytest.raises(KeyError):
        ix.find("no such entry")
    with zipfile.ZipFile(io.BytesIO(z)) as zf:
        cd = zf.start_dir
    assert ix.status.cd_off == cd


def test_small_cap_host():
    z = Z.cases()["count_65"]
    st, ent = Z.entry_array(z)
    L = D.lib()
    part = np.zeros(10, dtype=D.ZipEntryDTYPE)
    st2 = D.ZipStatus()
    buf = ctypes.create_string_buffer(z, len(z))
    assert L.dmx_zip_index_host(buf, len(z), ctypes.c_void_p(part.ctypes.data), 10, ctypes.byref(st2)) == 0
    assert st2.status == -E["E_SZ"] and st2.nentries == 65 and st2.out_len == st.out_len
    assert part.tobytes() == ent[:10].tobytes()
    assert L.dmx_zip_index_host(None, 5, None, 0, ctypes.byref(st2)) == INVAL
    assert L.dmx_zip_index_host(buf, len(z), None, 1, ctypes.byref(st2)) == INVAL
    assert L.dmx_zip_index_host(buf, len(z), None, 0, None) == INVAL


def test_comment_with_end_signature_is_refused():
    z = Z.comment_with_end_signature()
    with pytest.raises(zipfile.BadZipFile):
        zipfile.ZipFile(io.BytesIO(z))
    st, ent = Z.entry_array(z)
    assert st.status < 0 and st.nentries == 0 and len(ent) == 0
    with pytest.raises(D.DeflateError):
        D.zip_index(z)


@pytest.mark.parametrize("name", sorted(Z.corrupt_cases()))
def test_corrupt_statuses(name):
    base = Z.corrupt_cases()["base"][0]
    z, fstat, idx, estat = Z.corrupt_cases()[name]
    st0, ent0 = Z.entry_array(base)
    st, ent = Z.entry_array(z)
    assert st.status == fstat, name
    if fstat:
        assert st.nentries == 0 and st.out_len == 0
        return
    assert st.nentries == st0.nentries
    run = 0
    for i in range(st.nentries):
        a, b = ent[i], ent0[i]
        if i == idx:
            assert int(a["status"]) == estat, name
        else:   # every other entry is unchanged
            for f in ("data_off", "csize", "usize", "hdr_off", "name_off", "crc", "status", "method", "flags", "name_len"):
                assert a[f] == b[f], (name, i, f)
        assert int(a["out_off"]) == run
        run += 0 if int(a["status"]) else int(a["usize"])
    assert st.out_len == run


def test_empty_archive():
    z = Z.cases()["count_0"]
    assert len(z) == 22
    st, ent = Z.entry_array(z)
    assert (st.status, st.nentries, st.out_len, st.cd_off, st.cd_len) == (0, 0, 0, 0, 0)
    st, _ = Z.entry_array(b"")
    assert st.status == -E["E_ZHEAD"]


def test_host_twin_asan_ubsan(tmp_path):
    """tests/c/zip_model.cpp prints `0 failed checks`: on every archive of the case list (each at the
    alignments 0..15, with too few entries and with too small a candidate buffer) and, for two small
    archives, on every truncation and with every byte of the central directory and the end records
    set to 00 and FF, the stages of the device index, run as loops, give dmx_zip_index_host's record
    and entries."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.zip"])
    files = []
    everything = dict(Z.cases())
    everything["comment_sig"] = Z.comment_with_end_signature()
    for k, (z, _, _, _) in Z.corrupt_cases().items():
        everything["corrupt_" + k] = z
    for k, z in everything.items():
        f = tmp_path / f"{k}.zip"
        f.write_bytes(z)
        files.append(str(f))
    small = []
    for k, z in (("m_plain", Z.craft(Z.small_entries(4) + [Z.Ent("s", b"stored", 0)], comment=b"hi")),
                 ("m_zip64", Z.craft(Z.small_entries(3), zip64=True, prefix=b"xy"))):
        f = tmp_path / f"{k}.zip"
        f.write_bytes(z)
        small.append(str(f))
    exe = os.path.join(REPO, "build", "c", "zip_model")
    runs = [subprocess.Popen([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True),
            subprocess.Popen([exe, "--mutate"] + small, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)]
    for p in runs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, out[-2000:] + err[-4000:]
        assert " 0 failed checks" in out
