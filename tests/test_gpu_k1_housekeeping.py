"""The match kernel's per-block housekeeping on the MI355X: the Adler-32 sums
taken from the staging registers, the branch-free distance permute, and the DMX_F_DEEP
statistic taken from the counting sort's own hashes.

Bar: bit-exact.  Every case: the stream equals the oracle's byte for byte, the Adler-32 is
zlib's, and no block fell back to the exact sort.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import deflate_compression_amd as D  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.deep_inputs import bitdump  # noqa: E402
from tests.deep_threshold_inputs import pair  # noqa: E402

B = 32768


@pytest.fixture(scope="module")
def enc():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = D.Encoder(0, 8 << 20)
    yield e
    e.close()


@pytest.fixture(scope="module")
def text():
    return D.gen_text(4 * B, 0xAD1E).tobytes()


def _flags(lazy=True, deep=False, store_check=False, dict=False):
    return (D.DMX_ZLIB | (D.DMX_F_LAZY if lazy else 0) | (D.DMX_F_DEEP if deep else 0)
            | (D.DMX_F_STORE_CHECK if store_check else 0) | (D.DMX_F_DICT if dict else 0))


def check(enc, data, k=7, lazy=True, deep=False, store_check=False, dict=False, tag=None):
    """One encode against the oracle: stream, Adler-32, no sort fallback.  Returns the result."""
    z, r = enc.compress_bytes(data, max_chain=k, flags=_flags(lazy, deep, store_check, dict))
    assert r.status == 0, tag
    assert z == O.compress(data, max_chain=k, lazy=lazy, deep=deep, store_check=store_check, dict=dict), tag
    assert r.adler == zlib.adler32(data), tag
    assert r.nsortfallback == 0, tag
    return r


def check_tokens(enc, data, k, lazy, deep=False, dict=False, tag=None):
    """check(), then every block's tokens against the oracle's parse of that block."""
    check(enc, data, k=k, lazy=lazy, deep=deep, dict=dict, tag=tag)
    want = O.parse(data, max_chain=k, lazy=lazy, dict=dict, deep=deep)
    for b, w in enumerate(want):
        assert np.array_equal(enc.tokens(b), w), (tag, b)


def ff_block():
    """A full block of 0xFF with one 0x00: not uniform (it is staged and summed by K1), and
    the largest sums a block can produce."""
    a = bytearray(b"\xff" * B)
    a[12345] = 0
    return bytes(a)


# ---- Adler-32 from the staging registers ----

@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 33, 4095, 32767, 32768, 32769, 2 * 32768 + 5])
def test_adler_sizes(enc, text, n):
    check(enc, text[:n], tag=n)


def test_adler_largest_sums(enc, text):
    ff = ff_block()
    check(enc, ff, tag="ff")
    # the same block as the last, short block after two text blocks (its 0x00 still inside)
    check(enc, text[:2 * B] + ff[:20000], tag="ff tail")
    check(enc, ff + ff[:12346] + text[:100], tag="ff twice")


@pytest.mark.parametrize("shift", [1, 3, 8])
def test_adler_unaligned_input(enc, text, shift):
    """An input pointer that is not 16-byte aligned: the byte-wise staging path."""
    data = text[:B + 777] + ff_block() + text[B:B + 4097]
    buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    buf[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    t = buf[shift:shift + len(data)]
    assert t.data_ptr() % 16 == shift
    z, r = enc.compress_tensor(t, opts=D.Opts(B, 7, _flags(), 0))
    assert r.status == 0 and r.nsortfallback == 0
    assert z.cpu().numpy().tobytes() == O.compress(data, max_chain=7, lazy=True)
    assert r.adler == zlib.adler32(data)


def _mixed(text):
    return (text[:B + 100] + D.gen_random(2 * B, 5).tobytes() + bytes(B + 50) + ff_block()
            + D.gen_random(B, 6).tobytes() + text[B:2 * B + 333])


@pytest.mark.parametrize("store_check", [False, True])
def test_adler_mixed_blocks(enc, text, store_check):
    """Text, noise, zeros: with the noise check the result combines blocks summed by K0
    (stored), by K1's closed form (uniform) and by K1's staging loop."""
    check(enc, _mixed(text), store_check=store_check, deep=True, tag=store_check)


def test_adler_with_dict(enc, text):
    check(enc, text[:2 * B + 999] + ff_block() + text[:5000], dict=True, tag="dict")


@pytest.mark.parametrize("shape", ["list", "plain"])
def test_adler_both_launch_shapes(enc, text, shape):
    """K1 a workgroup per block and K1 looping over the work list (both instantiations share
    the staging loop); the threshold pair rides along, so the looping kernel takes the depth
    statistic from its sort too."""
    deep, shallow = pair()
    data = _mixed(text) + deep + shallow + deep[:3000]
    enc.set_hook("worklist", shape)
    try:
        for rep in range(2):
            check(enc, data, store_check=True, deep=True, tag=(shape, rep))
    finally:
        enc.set_hook("worklist", None)


# ---- the distance permute ----

def _permute_inputs(text):
    rng = np.random.default_rng(11)
    cases = {}
    for n in (3, 4, 10, 11, 1001, 1002, 1003, 32761, 32762, 32763):   # 8 q + 1, 2, 3 at q = 125 and 4095
        cases[f"text{n}"] = text[:n]
    half = text[:B // 2]
    cases["dist16384"] = half + half
    cases["dist32468"] = text[:300] + rng.integers(0, 256, B - 600, dtype=np.uint8).tobytes() + text[:300]
    cases["runs"] = bytes([5]) * 20000 + b"x" + bytes([6]) * 9000 + b"yz" + bytes([5]) * 3765
    # matchable and unmatched positions side by side: a phrase, then three random bytes
    alt = b"".join(b"HELLO" + rng.integers(0, 256, 3, dtype=np.uint8).tobytes() for _ in range(B // 8))
    cases["alternating"] = alt[:B - 5]
    return cases


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("k", [1, 4, 6, 7, 8, 16])
def test_permute_tokens(enc, text, k, lazy):
    """Tokens per block at every short-chain depth, and at K = 16 (distances staged in HBM)."""
    for name, data in _permute_inputs(text).items():
        check_tokens(enc, data, k, lazy, tag=(name, k, lazy))


@pytest.mark.parametrize("lazy", [False, True])
def test_permute_history_winners(enc, text, lazy):
    """DMX_F_DICT at K = 7 on two blocks, the second a repeat of the first: its winners are the
    history's (nibble 15)."""
    blk = text[:B]
    check_tokens(enc, blk + blk, 7, lazy, dict=True, tag=("dict", lazy))
    check_tokens(enc, blk + blk[:10003], 7, lazy, dict=True, tag=("dict short", lazy))


# ---- the depth statistic from the sort's hashes ----

@pytest.mark.parametrize("k", [7, 8])
def test_depth_threshold_pair(enc, k):
    """4 D = samples - 4 is deep, 4 D = samples is not (tests/test_deep_threshold.py pins the
    oracle's verdicts): alone and side by side in one launch."""
    deep, shallow = pair()
    check_tokens(enc, deep, k, True, deep=True, tag="deep")
    assert np.array_equal(enc.tokens(0), O.parse_block(deep, 32, lazy=True))
    check_tokens(enc, shallow, k, True, deep=True, tag="shallow")
    assert np.array_equal(enc.tokens(0), O.parse_block(shallow, k, lazy=True))
    check_tokens(enc, deep + shallow + shallow + deep, k, True, deep=True, tag="both")


@pytest.mark.parametrize("n", [2, 3, 255, 256, 258, 2048 + 3, 4096 + 2])
def test_depth_short_blocks(enc, text, n):
    """Short blocks, alone and as the tail after a full block: a bit dump (deep from 255 bytes
    on, tests/test_deep.py) and text (never deep)."""
    for name, src in (("bitdump", bitdump(B + n, 9)), ("text", text)):
        check_tokens(enc, src[:n], 7, True, deep=True, tag=(name, n))
        check_tokens(enc, src[:B] + src[:n], 6, False, deep=True, tag=(name, n, "tail"))


def test_depth_above_kd_asks_block_chain(enc):
    """dmx_opts.deep_chain above 32: the statistic comes from block_chain before the sort."""
    deep, shallow = pair()
    data = deep + shallow
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    O.set_deep_chain(48)
    try:
        z, r = enc.compress_tensor(t, opts=D.Opts(B, 7, _flags(deep=True), 48))
        assert r.status == 0 and r.nsortfallback == 0
        assert z.cpu().numpy().tobytes() == O.compress(data, max_chain=7, lazy=True, deep=True)
        assert r.adler == zlib.adler32(data)
        assert np.array_equal(enc.tokens(0), O.parse_block(deep, 48, lazy=True))
        assert np.array_equal(enc.tokens(1), O.parse_block(shallow, 7, lazy=True))
    finally:
        O.set_deep_chain(0)
