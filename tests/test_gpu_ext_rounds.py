"""The match extension's rounds on the MI355X (ext_len2 and the extension queue):
planted copies of every length around the rounds' ends (8 + 24, then every 32), at all 16
alignments of the two sides, with the mismatch in each byte of a word; copies cut by the end of
a full and of a short block; copies among the first entries of S; positions with three sources
whose lengths tie, differ by one, or cross a round end; copies whose source is in the previous
block (DMX_F_DICT, the history kernel's two-array use).  tests/test_ext_rounds_inputs.py shows
on the CPU that the oracle's token streams hold every plant.

Bar: bit-exact.  Every case: the stream equals the CPU oracle's (compress_par, same flags) byte
for byte, zlib inflates it, no block fell back to the exact sort, and the GPU's tokens hold
every plant.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import deflate_compression_amd as D  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import ext_rounds_inputs as X  # noqa: E402


@pytest.fixture(scope="module")
def enc():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = D.Encoder(0, 8 << 20)
    yield e
    e.close()


@pytest.fixture(scope="module")
def built():
    return X.build()


def check(enc, built, k, lazy, store_check=True, deep=True, dict=False):
    data, plants = built
    flags = (D.DMX_ZLIB | (D.DMX_F_LAZY if lazy else 0) | (D.DMX_F_DEEP if deep else 0)
             | (D.DMX_F_STORE_CHECK if store_check else 0) | (D.DMX_F_DICT if dict else 0))
    z, r = enc.compress_bytes(data, max_chain=k, flags=flags)
    assert r.status == 0 and r.nsortfallback == 0
    want = O.compress_par(data, max_chain=k, lazy=lazy, deep=deep, store_check=store_check, dict=dict)
    assert z == want
    assert zlib.decompress(z) == data
    assert r.adler == zlib.adler32(data)
    nblk = (len(data) + X.B - 1) // X.B
    assert r.nblocks == nblk
    assert X.find_plants([np.asarray(enc.tokens(b)) for b in range(nblk)], plants, dict) == []


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("k", [6, 7, 8])
def test_short_chain_quads(enc, built, k, lazy):
    """K = 6..8: four entries per lane, the extension queue's ring."""
    check(enc, built, k, lazy)


def test_store_check_off(enc, built):
    check(enc, built, 7, True, store_check=False, deep=False)


def test_one_entry_path(enc, built):
    """K = 4: an entry per lane, the queue flushed a chunk at a time."""
    check(enc, built, 4, True)


def test_long_chain_windows(enc, built):
    """K = 16: the register windows' extensions."""
    check(enc, built, 16, True)


def test_exhaustive(enc, built):
    check(enc, built, 0, False, store_check=False, deep=False)


@pytest.mark.parametrize("lazy", [False, True])
def test_history_kernel(enc, built, lazy):
    """DMX_F_DICT: the history kernel extends over two arrays (the block, the history)."""
    check(enc, built, 7, lazy, dict=True)
