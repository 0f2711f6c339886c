"""K3, the stream layout: the fused scan + apply launch and the three-launch scan
(the "scan3" hook) share one layout finish and one block apply, so they must agree in every
byte of the stream and in every field of dmx_result -- at the tile edges (256 blocks a tile),
in every container, with and without DMX_F_FINAL, with the work lists, on the empty input and
when the stream does not fit.

Bar: byte-equal streams and equal dmx_result records between the two paths; the streams
bit-exact against the oracle (zlib) or the gzip / BGZF tests' expectations built from it."""
import ctypes
import functools
import gzip
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import deflate_compression_amd as D  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_gpu_bgzf import EOF_MEMBER  # noqa: E402
from test_gpu_bgzf import _want as _want_bgzf  # noqa: E402
from test_gpu_gzip import _want as _want_gzip  # noqa: E402

SW = 256   # small blocks: 513 of them are 128 KiB
NBLK = [1, 255, 256, 257, 513]   # one tile less a block, a full tile, a block into the second, into the third
CONTAINERS = {"zlib": D.DMX_ZLIB, "gzip": D.DMX_GZIP, "bgzf": D.DMX_BGZF}
FIELDS = [f for f, _ in D.Result._fields_]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def enc():
    e = D.Encoder(0, NBLK[-1] * SW, sw=SW)
    yield e
    e.set_hook("scan3", 0)
    e.set_hook("worklist", None)
    e.close()


@functools.lru_cache(maxsize=None)
def _input(nblk: int) -> bytes:
    """nblk blocks of SW bytes, the last one ragged: zeros (fixed blocks) with runs of one to
    three blocks of text (dynamic) and of noise (stored) every five blocks, so blocks of every
    type lie next to each other and across the tile edges."""
    rng = np.random.default_rng(11 + nblk)
    a = np.zeros(nblk * SW - SW // 3, dtype=np.uint8)
    text = D.gen_text(8 * SW, 11)
    for s in range(0, nblk, 5):
        k = int(rng.integers(1, 4))
        e = min((s + k) * SW, a.size)
        m = e - s * SW
        if (s // 5) % 3 == 0:
            a[s * SW:e] = text[:m]
        elif (s // 5) % 3 == 1:
            a[s * SW:e] = rng.integers(0, 256, m, dtype=np.uint8)
    assert (a.size + SW - 1) // SW == nblk and a.size % SW
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def _want(nblk: int, container: str, final: bool, store_check: bool = False) -> bytes:
    """the expected stream: the oracle's (zlib), or what the gzip / BGZF tests build from it"""
    data = _input(nblk)
    if container == "bgzf":
        return _want_bgzf(data, sw=SW, fast="check" if store_check else False, final=final)
    o = O.compress(data, sw=SW, store_check=store_check, flags=O.F_HEADER | O.F_TRAILER | (O.F_FINAL if final else 0))
    return o if container == "zlib" else _want_gzip(data, o)


def _flags(container: str, final: bool) -> int:
    return CONTAINERS[container] if final else CONTAINERS[container] & ~D.DMX_F_FINAL


def _record(r) -> dict:
    return {f: int(getattr(r, f)) for f in FIELDS if f != "nsortfallback_total"}   # (the context's running total)


def _both_paths(enc, data, flags):
    """(stream, dmx_result) of the fused launch and of the three-launch scan"""
    got = []
    try:
        for v in (0, 1):
            enc.set_hook("scan3", v)
            z, r = enc.compress_bytes(data, sw=SW, flags=flags)
            got.append((z, _record(r)))
    finally:
        enc.set_hook("scan3", 0)
    return got


@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("container", sorted(CONTAINERS))
@pytest.mark.parametrize("nblk", NBLK)
def test_tile_edges(enc, nblk, container, final):
    data = _input(nblk)
    (z0, r0), (z1, r1) = _both_paths(enc, data, _flags(container, final))
    assert z0 == z1, (nblk, container, final)
    assert r0 == r1, (nblk, container, final)
    assert z0 == _want(nblk, container, final), (nblk, container, final)
    assert r0["status"] == 0 and r0["out_len"] == len(z0) and r0["nblocks"] == nblk and r0["n"] == len(data)
    assert r0["nstored"] + r0["nfixed"] + r0["ndynamic"] == nblk
    if nblk == 257:   # not a degenerate input: every block type, hence every kind of neighbour
        assert r0["nstored"] > 0 and r0["nfixed"] > 0 and r0["ndynamic"] > 0, r0
    if final and container == "zlib":
        assert zlib.decompress(z0) == data
    elif final:
        assert gzip.decompress(z0) == data


def test_with_work_lists(enc):
    """DMX_F_STORE_CHECK with the work lists (list-striding launches, and a workgroup per block
    with the skip): the apply's third path, on both scan paths"""
    data = _input(257)
    want = _want(257, "zlib", True, store_check=True)
    recs = []
    try:
        for shape in ("list", "plain"):
            enc.set_hook("worklist", shape)
            for z, r in _both_paths(enc, data, D.DMX_ZLIB | D.DMX_F_STORE_CHECK):
                assert z == want, shape
                recs.append(r)
    finally:
        enc.set_hook("worklist", None)
    assert all(r == recs[0] for r in recs), recs
    assert recs[0]["nstored"] > 0 and recs[0]["adler"] == zlib.adler32(data)


EMPTY = {
    ("zlib", True): bytes([0x78, 0x9C, 0x03, 0x00, 0x00, 0x00, 0x00, 0x01]),
    ("gzip", True): bytes([0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0, 0xFF, 0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0]),
    ("bgzf", True): EOF_MEMBER,
    ("bgzf", False): b"",
    # without DMX_F_FINAL an empty shard is its framing alone: no block, no sync flush
    ("zlib", False): bytes([0x78, 0x9C, 0x00, 0x00, 0x00, 0x01]),
    ("gzip", False): bytes([0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0, 0xFF, 0, 0, 0, 0, 0, 0, 0, 0]),
}


@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("container", sorted(CONTAINERS))
def test_empty_input(enc, container, final):
    """n = 0 has no tile: the one-workgroup scan writes the whole stream, whatever the hook"""
    (z0, r0), (z1, r1) = _both_paths(enc, b"", _flags(container, final))
    assert z0 == z1 == EMPTY[container, final], (container, final, z0.hex())
    assert r0 == r1 and r0["status"] == 0 and r0["out_len"] == len(z0) and r0["nblocks"] == 0
    if final:
        assert (zlib.decompress(z0) if container == "zlib" else gzip.decompress(z0)) == b""


@pytest.mark.parametrize("container", sorted(CONTAINERS))
def test_capacity_on_both_paths(enc, container):
    """a stream 4 bytes too long for out_cap: -E_SZ with the true length in the result, and
    nothing written at or beyond out_cap, on both scan paths"""
    data = _input(257)
    want = _want(257, container, True)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    o = D.Opts(SW, 0, CONTAINERS[container], 0)
    cap = (len(want) - 4) & ~3
    room = D.max_compressed(len(data), SW, CONTAINERS[container]) + 64
    enc.reserve(len(data), SW)
    try:
        for v in (0, 1):
            enc.set_hook("scan3", v)
            out = torch.full((room,), SENTINEL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()   # (the encode runs on the context's own stream)
            enc.encode_async(t.data_ptr(), len(data), out.data_ptr(), cap, None, o)
            r = D.Result()
            assert enc._L.dmx_encode_result(enc._ctx, ctypes.byref(r), None) == 0
            assert r.status == -D.E["E_SZ"] and r.out_len == len(want), (container, v, r.status, r.out_len)
            assert bool((out[cap:] == SENTINEL).all()), (container, v)
    finally:
        enc.set_hook("scan3", 0)
