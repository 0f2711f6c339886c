"""GPU inflate (csrc/dmx_inflate_dev.hip) on the hand-built corpus of deflate_craft.py, through
its three decode paths: the stream kernel, the indexed kernel with its 8 KiB ring, and the
cell kernel of the chained decode.  zlib's bytes are the reference of the valid cases; the
host decoder's status (deflate_decompress, called here) is the reference of the invalid ones
and of every truncated or bit-flipped stream -- both decoders implement one status contract
(include/dmx.h).  Every launch is one workgroup on at most a few tens of KiB.
"""
import numpy as np
import pytest
import torch

import deflate_compression_amd as D
import deflate_craft as C
from test_inflate_conformance import _host, flipped_streams, truncation_status

pytestmark = pytest.mark.gpu

CAP = 1 << 20   # more than any stream of a few hundred bytes can decode to, so -E_SZ never hides a status
VALID = [n for n, _, k in C.CASES if k == "valid"]
INVALID = [n for n, _, k in C.CASES if k == "invalid"]
_dev_cache = {}


def _dev(b: bytes, lead: int = 0):
    """b on the device, `lead` bytes into a 256-byte aligned allocation."""
    t = torch.frombuffer(bytearray(bytes(lead) + b), dtype=torch.uint8).cuda()
    return t[lead:]


def _case(name):
    if name not in _dev_cache:
        _dev_cache[name] = _dev(C.zstream(name))
    return _dev_cache[name]


def _index(entries):
    """dmx_iblock records {u64 bit, u64 out_off, u32 out_len, u32 reserved} on the device."""
    a = np.zeros(len(entries), dtype=[("bit", "<u8"), ("off", "<u8"), ("len", "<u4"), ("res", "<u4")])
    for k, e in enumerate(entries):
        a[k] = (*e, 0)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def _stream(name):
    want = C.expected(name)
    dec, st = D.inflate_gpu(_case(name), len(want) + 16 if name in VALID else CAP)
    return dec.cpu().numpy().tobytes(), st


def _indexed(name, chained):
    """One sw block from bit 16: out_len the expected length (1024 for an invalid case)."""
    want = C.expected(name)
    olen = len(want) if name in VALID else 1024
    ix = _index([(16, 0, olen)])
    f = D.inflate_gpu_chained if chained else D.inflate_gpu
    dec, st = f(_case(name), olen + 16, ix, 1)
    return dec.cpu().numpy().tobytes(), st


def _check_valid(run, names):
    bad = []
    for name in names:
        got, st = run(name)
        if st != 0 or got != C.expected(name):
            bad.append((name, st, len(got), len(C.expected(name))))
    assert not bad, bad


def test_valid_stream():
    _check_valid(_stream, VALID)


def test_valid_indexed():
    names = [n for n in VALID if n not in C.STREAM_ONLY]
    assert "stored32510_dist32507" in names and len(names) >= 20
    _check_valid(lambda n: _indexed(n, False), names)


def test_valid_chained():
    _check_valid(lambda n: _indexed(n, True), [n for n in VALID if n not in C.STREAM_ONLY])


def test_far_window_as_two_chained_blocks():
    """A stored block of history and a fixed block whose one match starts 32768 (32767, 32507)
    bytes back, decoded as two sw blocks: the match lies wholly before its block."""
    bad = []
    for name, hist in C.TWO_BLOCK.items():
        want = C.expected(name)
        ix = _index([(16, 0, hist), (16 + 8 * (5 + hist), hist, len(want) - hist)])
        dec, st = D.inflate_gpu_chained(_case(name), len(want) + 16, ix, 2)
        if st != 0 or dec.cpu().numpy().tobytes() != want:
            bad.append((name, st, dec.numel()))
    assert not bad, bad


def _host_status(name):
    out, st = _host(C.zstream(name))
    assert st == -D.E[C.STATUS[name]], (name, st)   # (the host's own test says the same)
    return st


def test_invalid_stream():
    bad = []
    for name in INVALID:
        _, st = _stream(name)
        want = _host_status(name)
        if st != want:
            bad.append((name, st, want))
    assert not bad, bad


@pytest.mark.parametrize("chained", [False, True])
def test_invalid_indexed(chained):
    """The same status where the error precedes any output (tables, headers, BTYPE, LEN/NLEN,
    a first symbol); a negative one otherwise (out_len 1024 may end the block first)."""
    bad = []
    for name in INVALID:
        if name in C.STREAM_ONLY:
            continue
        _, st = _indexed(name, chained)
        want = _host_status(name)
        if (st != want) if name in C.EARLY else (st >= 0):
            bad.append((name, st, want))
    assert not bad, bad


@pytest.mark.parametrize("which", ["fixed", "dynamic", "stored"])
def test_truncation_sweep(which):
    """Every prefix as a view of the full device buffer: a reader that runs past zbytes finds
    the rest of the stream there and shows up as a wrong status, not as a fault."""
    z, data = C.sweep_streams()[which]
    zd = _dev(z)
    dec, st = D.inflate_gpu(zd, CAP)
    assert st == 0 and dec.cpu().numpy().tobytes() == data
    with pytest.raises(D.DeflateError) as ei:   # no bytes at all: a null view, refused at the boundary
        D.inflate_gpu(zd[:0], CAP)
    assert ei.value.code == -D.E["E_INVAL"]
    bad = []
    for k in range(1, len(z)):
        _, st = D.inflate_gpu(zd[:k], CAP)
        want = _host(z[:k])[1]
        assert want == truncation_status(z, k)
        if st != want:
            bad.append((k, st, want))
    assert not bad, bad


def test_bitflip_sweep():
    """200 single-bit flips: the host's status (zlib's verdict, test_host_bitflip_sweep), and
    zlib's bytes where the flip is accepted.  The streams start 0..3 bytes off a dword."""
    z, data, flips = flipped_streams()
    bad = []
    for k, c in enumerate(flips):
        dec, st = D.inflate_gpu(_dev(c, k % 4), CAP)
        got, want = _host(c)
        if st != want or (st == 0 and dec.cpu().numpy().tobytes() != got):
            bad.append((k, st, want))
    assert not bad, bad
