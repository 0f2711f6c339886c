"""The segment walk of K1's greedy path on the MI355X (W1, the Jacobi rounds, W2, W3 and the
one-lane walk; csrc/dmx_walk.h): planted copies at the segment offsets the walk
distinguishes -- a literal run up to a segment end with a match at offset 0 behind it, matches
that start at offset 31, end on a boundary, span eight segments or end at bn, whole segments of
literals, lazy pairs and chains of three across a boundary, last blocks of 1 .. 32767 bytes --
and two periodic blocks that take the one-lane walk (rounds stopped at 3) and the per-wave
resolution (8 rounds without a fixed point).  tests/test_walk_inputs.py shows on the CPU that
the oracle's token streams hold every plant.

Bar: bit-exact.  Every case: the stream equals the CPU oracle's (compress_par, same settings)
byte for byte, zlib inflates it, no block fell back to the exact sort, and the GPU's tokens hold
every plant.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import deflate_compression_amd as D  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import walk_paths_inputs as W  # noqa: E402

BUILT = W.build() + [("period-37", W.periodic_block(0), []), ("period-37-behind-2048", W.periodic_block(2048), [])]
NAMES = [name for name, _, _ in BUILT]


@pytest.fixture(scope="module")
def enc():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = D.Encoder(0, 8 << 20)
    yield e
    e.close()


_want = {}


def oracle_stream(name, data, **kw):
    """The oracle's stream of one input at one setting, computed once."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _want:
        _want[key] = O.compress_par(data, **kw)
    return _want[key]


def check(enc, case, k, lazy, store_check=False, dict=False):
    name, data, plants = case
    flags = (D.DMX_ZLIB | (D.DMX_F_LAZY if lazy else 0) | (D.DMX_F_STORE_CHECK if store_check else 0)
             | (D.DMX_F_DICT if dict else 0))
    z, r = enc.compress_bytes(data, max_chain=k, flags=flags)
    assert r.status == 0 and r.nsortfallback == 0
    assert z == oracle_stream(name, data, max_chain=k, lazy=lazy, store_check=store_check, dict=dict)
    assert zlib.decompress(z) == data
    nblk = (len(data) + W.B - 1) // W.B
    assert r.nblocks == nblk
    if plants and not store_check:   # (a stored block has no tokens)
        assert W.find_plants([np.asarray(enc.tokens(b)) for b in range(nblk)], plants, lazy) == []


@pytest.mark.parametrize("lazy", [False, True], ids=["greedy", "lazy"])
@pytest.mark.parametrize("case", BUILT, ids=NAMES)
def test_k7(enc, case, lazy):
    check(enc, case, 7, lazy)


def test_store_check_on(enc):
    for case in BUILT:
        check(enc, case, 7, True, store_check=True)


def test_long_chain(enc):
    for case in BUILT:
        check(enc, case, 16, True)


def test_exhaustive(enc):
    for case in BUILT:
        check(enc, case, 0, True)


def test_history(enc):
    for case in BUILT:
        check(enc, case, 7, True, dict=True)


@pytest.mark.parametrize("lazy", [False, True], ids=["greedy", "lazy"])
@pytest.mark.parametrize("head,rounds", [(0, 3), (2048, 8)], ids=["one-lane-walk", "per-wave-resolution"])
def test_periodic_block_paths(monkeypatch, head, rounds, lazy):
    """Shapes 9 and 10: every position holds a 258-byte match, so the rounds find no fixed
    point.  Fewer than 1024 tokens: the rounds stop at 3 for the one-lane walk.  More (2048
    random bytes first): all 8 rounds run, then W2 and W3.  The stamps say which path ran."""
    monkeypatch.setenv("DMX_STAMPS", "1")
    data = W.periodic_block(head)
    flags = D.DMX_ZLIB | (D.DMX_F_LAZY if lazy else 0)
    e = D.Encoder(0, 1 << 20)
    try:
        z, r = e.compress_bytes(data, max_chain=7, flags=flags)
        st = e.stamps(1)
        tok = np.asarray(e.tokens(0))
    finally:
        e.close()
    assert r.status == 0 and r.nsortfallback == 0 and r.nblocks == 1
    assert int(st[0, 11]) == rounds, st[0, 11]
    assert z == O.compress_par(data, max_chain=7, lazy=lazy)
    assert zlib.decompress(z) == data
    assert np.array_equal(tok, O.parse(data, max_chain=7, lazy=lazy)[0])
    assert (len(tok) < 1024) == (head == 0)
