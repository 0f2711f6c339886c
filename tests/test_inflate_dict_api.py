"""Preset dictionaries without a device: the exports and declarations of dmx_inflate_batch_dict_async,
dmx_bdict, the argument errors the call returns before any device call, the size of its work buffer,
the host twin of its framing (tests/c/frame_dict_model.cpp: dmx_frame_head_dict against
dmx_inflate_dict_host under ASan + UBSan, a stand-alone program), and the host decoder against
zlib.decompressobj(wbits, zdict=d) on every case of inflate_dict_inputs."""
import ctypes
import os
import subprocess

import pytest

import deflate_compression_amd as D
import inflate_dict_inputs as I

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE = -E["E_INVAL"], -E["E_RANGE"]
vp = ctypes.c_void_p


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in ("dmx_inflate_batch_dict_work", "dmx_inflate_batch_dict_async", "dmx_inflate_dict_host"):
        f = getattr(L, name)
        assert f.argtypes is not None, name
        assert name + "(" in hdr, name
    for name in ("dmx_bdict", "DMX_BATCH_NODICT 0xFFFFFFFFu", "inflateSetDictionary"):
        assert name in hdr, name
    for name in ("inflate_batch_dict_async", "inflate_dict_host", "BDict", "DMX_BATCH_NODICT"):
        assert name in D.__all__ and hasattr(D, name), name
    assert D.DMX_BATCH_NODICT == 0xFFFFFFFF
    import inspect
    sig = inspect.signature(D.inflate_batch)
    assert sig.parameters["zdict"].default is None and sig.parameters["dict_of"].default is None


def test_struct_size():
    assert ctypes.sizeof(D.BDict) == 16
    assert [getattr(D.BDict, f).offset for f, _ in D.BDict._fields_] == [0, 8]


def _call(z=0x1000, zbytes=64, streams=0x2000, n=3, flags=0, dic=0x6000, dict_bytes=64, dicts=0x7000, ndicts=2,
          dict_of=0x8000, out=0x3000, out_bytes=64, results=0x4000, work=0x10000, work_bytes=None, status=0x5000):
    """dmx_inflate_batch_dict_async on made-up addresses: an argument error returns before they are used"""
    L = D.lib()
    if work_bytes is None:
        work_bytes = L.dmx_inflate_batch_dict_work(n, ndicts)
    return L.dmx_inflate_batch_dict_async(vp(z), zbytes, vp(streams), n, flags, vp(dic), dict_bytes, vp(dicts), ndicts,
                                          vp(dict_of), vp(out), out_bytes, vp(results), vp(work), work_bytes, vp(status), vp(0))


def test_argument_errors():
    L = D.lib()
    need = L.dmx_inflate_batch_dict_work(3, 2)
    assert _call(results=0) == INVAL
    assert _call(status=0) == INVAL
    assert _call(work=0) == INVAL
    assert _call(streams=0) == INVAL                    # NULL with nstreams > 0
    assert _call(z=0) == INVAL                          # NULL with zbytes > 0
    assert _call(out=0) == INVAL                        # NULL without the measure flag
    for fmt in (0, 1, 2, 3):
        assert _call(out=0, flags=fmt) == INVAL
    assert _call(streams=0x2004) == INVAL               # 8-byte alignment of the descriptors
    assert _call(results=0x4004) == INVAL
    assert _call(status=0x5004) == INVAL
    assert _call(work=0x10080) == INVAL                 # 256-byte alignment of the work buffer
    assert _call(work_bytes=need - 1) == INVAL
    assert _call(work_bytes=L.dmx_inflate_batch_work(3)) == INVAL   # the old size is too small with dictionaries
    assert _call(work_bytes=0) == INVAL
    assert _call(dicts=0) == INVAL                      # NULL with ndicts > 0
    assert _call(dic=0) == INVAL                        # NULL with dict_bytes > 0
    assert _call(dicts=0x7004) == INVAL                 # 8-byte alignment of the dictionary records
    for a in (1, 2, 3):
        assert _call(dict_of=0x8000 + a) == INVAL       # 4-byte alignment of the indices
    for flags in (4, 15, 32, 3 | 32, 16 | 7, 0x80000000, 0x100):
        assert _call(flags=flags) == RANGE, flags
    assert _call(status=0, flags=32) == INVAL           # a NULL beats a bad flag


def test_work_size():
    L = D.lib()
    for n in (0, 1, 3, 64, 2047, 2048, 4096, 1 << 20, 0xFFFFFFFF):
        assert L.dmx_inflate_batch_dict_work(n, 0) == L.dmx_inflate_batch_work(n), n
        last = 0
        for nd in (0, 1, 2, 63, 64, 65, 1024, 1 << 20, 0xFFFFFFFF):
            w = L.dmx_inflate_batch_dict_work(n, nd)
            assert w % 256 == 0 and w >= last and w >= L.dmx_inflate_batch_work(n) + 4 * nd, (n, nd, w)
            last = w
    last = 0
    for n in (0, 1, 2, 3, 63, 64, 255, 256, 1023, 1024, 1025, 2047, 2048, 4096, 1 << 20, 0xFFFFFFFF):
        w = L.dmx_inflate_batch_dict_work(n, 7)
        assert w >= last, n
        last = w


def test_host_twin_asan_ubsan():
    """tests/c/frame_dict_model.cpp ends with `0 failed checks`: over every cut point of an FDICT
    header (and of a raw, a plain zlib and a gzip stream), every FLG, and 6 000 seeded header
    mutations, with no, the right, a wrong and an empty dictionary under all four formats, the verdict
    of the framing text the kernel runs is dmx_inflate_dict_host's status, and where it is 0 the host
    decodes the same bytes from the offset it names with the window primed exactly when it says so."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.frame_dict"])
    exe = os.path.join(REPO, "build", "c", "frame_dict_model")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert " checks, 0 failed checks" in p.stdout


def test_host_decoder_equals_zlib():
    bad = []
    for c in I.all_cases():
        try:
            got = D.inflate_dict_host(c.z, c.d, I.FMT_NAME[c.ask])
            status = 0
        except D.DeflateError as e:
            got, status = None, e.code
        if status != c.status or (status == 0 and got != (c.want, c.used)):
            bad.append((c.name, status, c.status, got and (len(got[0]), got[1]), c.want and (len(c.want), c.used)))
    assert not bad, bad[:10]
    assert len(I.all_cases()) > 80


def test_host_decoder_arguments():
    L = D.lib()
    out, n, used = vp(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    z = ctypes.create_string_buffer(b"\x03\x00", 2)
    args = (ctypes.byref(out), ctypes.byref(n), ctypes.byref(used))
    assert L.dmx_inflate_dict_host(z, 2, 4, None, 0, *args) == INVAL           # a format above 3
    assert L.dmx_inflate_dict_host(None, 2, 3, None, 0, *args) == INVAL
    assert L.dmx_inflate_dict_host(z, 2, 3, None, 5, *args) == INVAL           # NULL with dict_len > 0
    assert L.dmx_inflate_dict_host(z, 2, 3, None, 0, None, ctypes.byref(n), None) == INVAL
    assert L.dmx_inflate_dict_host(z, 2, 3, None, 0, ctypes.byref(out), ctypes.byref(n), None) == 0 and n.value == 0
    D._libc.free(out)
    with pytest.raises(ValueError):
        D.inflate_dict_host(b"", None, "lzma")
