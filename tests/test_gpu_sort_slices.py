"""K1's P0 on the MI355X: the counting sort's slices (csrc/dmx_sort_slices.h: the wave that ranks
a position range is not the wave of the same index) at every length at which a
slice or a group begins, ends or is cut short, and the uniform-block test that precedes the sort
(two votes: every thread's chunks are one byte; that byte is byte 0) at its edges.  Single blocks
of at most 32 KiB.

Bar: bit-exact.  Every case: the stream equals the CPU oracle's (compress_par, same settings)
byte for byte, zlib inflates it, and no block fell back to the exact sort -- but for the one
DMX_F_EXACT_SORT case, which asks for the fallback: there every block takes it once.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import deflate_compression_amd as D  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.deep_inputs import bitdump  # noqa: E402

B = 32768
SLICE = 2048
TRI = b"\xf0\xf1\xf2"   # bytes the text generator never writes: one bucket, these entries only
LENGTHS = (1, 2, 3, 2047, 2048, 2049, 4095, 4097, 8191, 8192, 8193, 16385, 32767, 32768)


def _text(n, seed=0x51CE):
    return D.gen_text(max(n, 1), seed).tobytes()[:n]


def _planted(slices):
    """A text block with TRI every 61 bytes inside the given slices: the bucket's entries lie
    in exactly those slices, about 33 in each."""
    a = bytearray(_text(B))
    assert TRI[0] not in a and TRI[1] not in a and TRI[2] not in a
    for s in slices:
        for p in range(s * SLICE + 7, (s + 1) * SLICE - 3, 61):
            a[p:p + 3] = TRI
    return bytes(a)


def _runny():
    """Runs of one byte in more than a quarter of the 16-byte chunks (the run-aware ranks), text
    between them, nothing uniform."""
    t = _text(B)
    parts = [bytes(5000), t[:6000], b"a" * 4099, t[6000:9000], b"\xff" * 3001, t[9000:]]
    return b"".join(parts)[:B]


def _inputs():
    out = [(f"len-{n}", _text(n)) for n in LENGTHS]
    out.append(("trigram-every-61", _planted(range(16))))
    out.append(("trigram-at-group-edges", _planted((3, 4, 7, 8, 11, 12))))
    out.append(("run-dominated", _runny()))
    return out


INPUTS = _inputs()
NAMES = [name for name, _ in INPUTS]


def _uniform_inputs():
    one = b"u" * B
    out = [("one-byte", one)]
    for p in (0, B - 1, 5, 2048 * 7 + 5, 2048 * 15 + 5):
        a = bytearray(one)
        a[p] = ord("v")
        out.append((f"other-byte-at-{p}", bytes(a)))
    # every 16-byte chunk is one byte, chunks alternate: a thread's own chunks (tid and
    # tid + 1024) agree, its neighbour's differ -- the first vote holds, the second must fail
    out.append(("chunks-alternate", b"".join(bytes([ord("a") + (c & 1)]) * 16 for c in range(B // 16))))
    out += [(f"one-byte-{n}", b"u" * n) for n in (1, 15, 16, 17, 32767)]
    return out


UNIFORM = _uniform_inputs()


@pytest.fixture(scope="module")
def enc():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = D.Encoder(0, 1 << 20)
    yield e
    e.close()


_want = {}


def oracle_stream(name, data, **kw):
    """The oracle's stream of one input at one setting, computed once."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _want:
        _want[key] = O.compress_par(data, **kw)
    return _want[key]


def check(enc, case, k, lazy, store_check=False, deep=False, exact=False):
    name, data = case
    flags = (D.DMX_ZLIB | (D.DMX_F_LAZY if lazy else 0) | (D.DMX_F_STORE_CHECK if store_check else 0)
             | (D.DMX_F_DEEP if deep else 0) | (D.DMX_F_EXACT_SORT if exact else 0))
    z, r = enc.compress_bytes(data, max_chain=k, flags=flags)
    assert r.status == 0 and r.nblocks == 1
    assert r.nsortfallback == (1 if exact else 0), (name, r.nsortfallback)
    assert z == oracle_stream(name, data, max_chain=k, lazy=lazy, store_check=store_check, deep=deep), name
    assert zlib.decompress(z) == data


def test_inputs_are_what_they_claim():
    """The planted trigram's positions by slice, and the run-dominated block's chunk count."""
    for name, want in (("trigram-every-61", set(range(16))), ("trigram-at-group-edges", {3, 4, 7, 8, 11, 12})):
        data = dict(INPUTS)[name]
        at, p = set(), data.find(TRI)
        while p >= 0:
            at.add(p // SLICE)
            assert (p + 2) // SLICE == p // SLICE
            p = data.find(TRI, p + 1)
        assert at == want
    r = np.frombuffer(dict(INPUTS)["run-dominated"], dtype=np.uint8).reshape(-1, 16)
    assert 4 * int((r == r[:, :1]).all(axis=1).sum()) >= B // 16 and len(set(dict(INPUTS)["run-dominated"])) > 2


@pytest.mark.parametrize("lazy", [False, True], ids=["greedy", "lazy"])
@pytest.mark.parametrize("case", INPUTS, ids=NAMES)
def test_k7(enc, case, lazy):
    check(enc, case, 7, lazy)


def test_long_chain_bucket_starts(enc):
    for case in INPUTS:
        check(enc, case, 16, True)


def test_exhaustive_four_byte_sort(enc):
    for case in INPUTS:
        check(enc, case, 0, True)


def test_deep_statistic_in_the_sort(enc):
    """DMX_F_DEEP at K = 7: the sort takes the depth statistic along.  The small-alphabet block
    takes the deep depth, the text block does not (the oracle's rule says which)."""
    small, text = bitdump(B, 1), _text(B)
    assert O.block_chain(small, 7) != 7 and O.block_chain(text, 7) == 7
    for case in [("deep-bitdump", small), ("deep-bitdump-4097", bitdump(4097, 4))] + INPUTS:
        check(enc, case, 7, True, deep=True)
        check(enc, case, 7, True, deep=True, store_check=True)


def test_exact_sort_fallback(enc):
    check(enc, ("trigram-every-61", dict(INPUTS)["trigram-every-61"]), 7, True, exact=True)


@pytest.mark.parametrize("store_check", [False, True], ids=["plain", "store-check"])
@pytest.mark.parametrize("case", UNIFORM, ids=[name for name, _ in UNIFORM])
def test_uniform_block_vote(enc, case, store_check):
    check(enc, case, 7, True, store_check=store_check)
    check(enc, case, 7, False, store_check=store_check)
