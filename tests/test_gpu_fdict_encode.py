"""DMX_F_FDICT on the single encode: a DMX_F_DICT stream whose zlib header names its dictionary
(78 BB and the DICTID, RFC 1950 2.2), so that zlib and this project's own batch decoder can be
handed the dictionary.  The DEFLATE data is that of the same encode without the flag; zlib is the
reference for the round trip.  Inputs of 1 B, 4 KiB and 100 KiB against dictionaries of 1, 300 and
32 768 bytes; the argument errors; the size bound.
"""
import ctypes
import os
import struct
import zlib

import pytest
import torch

import deflate_compression_amd as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    # torch opens the device before the library's host calls do (D.compress runs without torch)
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.init()

INVAL = -D.E["E_INVAL"]
SIZES = [1, 4096, 100 * 1024]
_text = {}


def _data(n):
    if n not in _text:
        _text[n] = D.gen_text(n, 21).tobytes()
    return _text[n]


def _pre(n):
    # text of the same generator (another seed), so matches into it exist
    if ("pre", n) not in _text:
        _text[("pre", n)] = D.gen_text(n, 22).tobytes()
    return _text[("pre", n)]


@pytest.mark.parametrize("plen", [1, 300, 32768])
@pytest.mark.parametrize("n", SIZES)
def test_fdict_stream(n, plen):
    data, d = _data(n), _pre(plen)
    z = D.compress(data, dict=True, pre=d, fdict=True)
    raw = D.compress(data, dict=True, pre=d, flags=D.DMX_F_FINAL | D.DMX_F_DICT)
    want = b"\x78\xbb" + struct.pack(">I", zlib.adler32(d)) + raw + struct.pack(">I", zlib.adler32(data))
    assert z == want
    o = zlib.decompressobj(zdict=d)
    assert o.decompress(z) == data and o.eof and not o.unused_data
    out, offs, res = D.inflate_batch([z], zdict=d)
    assert out.cpu().numpy().tobytes() == data
    assert (int(res["status"][0]), int(res["out_len"][0]), int(res["in_used"][0])) == (0, n, len(z))
    assert D.inflate_dict_host(z, d) == (data, len(z))
    if n == 4096 and plen == 32768:
        # the dictionary is used, not merely accepted
        assert len(z) < len(D.compress(data))
    # through a device-resident encode too (Encoder.compress_bytes via flags)
    enc = D.Encoder(0, n)
    try:
        z2, r = enc.compress_bytes(data, flags=D.DMX_ZLIB | D.DMX_F_DICT | D.DMX_F_FDICT, pre=d)
        assert r.status == 0 and z2 == want
    finally:
        enc.close()


def test_fdict_with_other_parse_options_and_small_windows():
    data, d = _data(100 * 1024), _pre(300)
    for kw in (dict(lazy=True), dict(store_check=True), dict(max_chain=7, lazy=True, deep=True), dict(sw=1024), dict(sw=300)):
        z = D.compress(data, dict=True, pre=d, fdict=True, **kw)
        assert z[:6] == b"\x78\xbb" + struct.pack(">I", zlib.adler32(d)), kw
        assert zlib.decompressobj(zdict=d).decompress(z) == data, kw
    # noise: stored blocks from the first one on (the speculative copy's offsets follow the header)
    noise = D.gen_random(100 * 1024, 3).tobytes()
    z = D.compress(noise, dict=True, pre=d, fdict=True, store_check=True)
    assert zlib.decompressobj(zdict=d).decompress(z) == noise


def _host(data, flags, pre, sw=32768, dict_len=None):
    """dmx_encode_host with the flags as given: its return code"""
    L = D.lib()
    p, n, keep = D._buf(data)
    cap = D.max_compressed(n, sw, flags)
    out = ctypes.create_string_buffer(cap)
    olen = ctypes.c_uint64(0)
    o = D.Opts(sw, 0, flags, 0)
    pk = None
    if pre is not None:
        pk = ctypes.create_string_buffer(bytes(pre), max(len(pre), 1))
        o.dict, o.dict_len = ctypes.cast(pk, ctypes.c_void_p), len(pre) if dict_len is None else dict_len
    r = L.dmx_encode_host(p, n, out, cap, ctypes.byref(olen), ctypes.byref(o))
    del keep, pk
    return r


def test_invalid_combinations():
    data, d = _data(4096), _pre(300)
    Z, DICT, FD = D.DMX_ZLIB, D.DMX_F_DICT, D.DMX_F_FDICT
    assert _host(data, Z | DICT | FD, d) == 0
    assert _host(data, Z | FD, d) == INVAL                                   # without DMX_F_DICT
    assert _host(data, D.DMX_F_FINAL | D.DMX_F_TRAILER | DICT | FD, d) == INVAL   # without DMX_F_HEADER
    assert _host(data, D.DMX_F_FINAL | DICT | FD, d) == INVAL
    assert _host(data, D.DMX_GZIP | DICT | FD, d) == INVAL                   # gzip has no DICTID
    assert _host(data, D.DMX_BGZF | FD, d) == INVAL
    assert _host(data, D.DMX_BGZF | DICT | FD, d) == INVAL
    assert _host(data, Z | DICT | FD, None) == INVAL                         # no dictionary
    assert _host(data, Z | DICT | FD, d, dict_len=0) == INVAL                # an empty one
    assert _host(data, Z | DICT | FD, _pre(32768) + b"x") == INVAL           # longer than sw
    assert _host(data, Z | DICT | FD, d, sw=256) == INVAL
    assert _host(data, Z | DICT | FD, d, sw=300) == 0                        # dict_len == sw
    with pytest.raises(D.DeflateError) as ei:
        D.compress(data, dict=True, fdict=True)
    assert ei.value.code == INVAL
    # a device-resident encode: the same rule in dmx_encode_async
    enc = D.Encoder(0, 4096)
    try:
        for flags, pre in ((Z | FD, d), (Z | DICT | FD, None), (Z | DICT | FD, _pre(32768) + b"x"), (D.DMX_GZIP | DICT | FD, d)):
            with pytest.raises(D.DeflateError) as ei:
                enc.compress_bytes(data, flags=flags, pre=pre)
            assert ei.value.code == INVAL, (flags, pre and len(pre))
    finally:
        enc.close()
    # the fd path and the batch encode refuse the flag
    L = D.lib()
    o = D.Opts(32768, 0, Z | DICT | FD, 0)
    rfd, wfd = os.pipe()
    try:
        devs = (ctypes.c_int * 1)(0)
        assert L.dmx_encode_fd_multi(rfd, wfd, ctypes.byref(o), 1 << 20, devs, 1) == INVAL
        two = (ctypes.c_int * 2)(0, 0)
        assert L.dmx_encode_fd_multi(rfd, wfd, ctypes.byref(o), 1 << 20, two, 2) == INVAL
    finally:
        os.close(rfd)
        os.close(wfd)
    with pytest.raises(D.DeflateError) as ei:
        D.compress_batch([data, data], flags=FD)
    assert ei.value.code == INVAL


def test_max_compressed_is_four_more():
    for n in (0, 1, 4096, 100 * 1024, 1 << 30):
        for sw in (32768, 1024):
            assert D.max_compressed(n, sw, D.DMX_ZLIB | D.DMX_F_DICT | D.DMX_F_FDICT) == D.max_compressed(n, sw, D.DMX_ZLIB | D.DMX_F_DICT) + 4
    assert D.DMX_F_FDICT == 2048 and "DMX_F_FDICT" in D.__all__
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dmx.h")).read()
    assert "#define DMX_F_FDICT 2048u" in hdr
