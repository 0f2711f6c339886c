"""K2 (dmx_huff_kernel) on the MI355X on the blocks of tests/k2_inputs.py: codes longer than their
limit in each alphabet (the overflow redistribution and the length assignment after it, DESIGN.md
§4.1), run-length classes of the header (§4.3) and the block type's two tie rules (§4.4).

Bar: bit-exact.  Tokens first (so that a K1 difference is not blamed on K2), then the block
type, the code lengths against the oracle's plan and against §4.1 themselves, the header as it
was emitted against RFC 1951 (tests/test_k2_inputs.check_header: not against the oracle), the
stream byte for byte, and both host inflates.  tests/test_k2_inputs.py shows on the CPU that
every block does what it is here for.
"""
import gzip
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import deflate_craft as C  # noqa: E402
import deflate_compression_amd as D  # noqa: E402
import k2_inputs as K  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_k2_inputs import CODE_CASES, check_header, check_lengths  # noqa: E402

OVERFLOW = sorted(set(K.OVERFLOW_LL) | {K.SHUFFLE} | set(K.OVERFLOW_D))


@pytest.fixture(scope="module")
def enc():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = D.Encoder(0, 1 << 20)
    e.reserve(1 << 20, 32768, D.DMX_F_SPLIT)
    yield e
    e.close()


@pytest.mark.parametrize("name,k,lazy", CODE_CASES)
def test_codes_and_header(enc, name, k, lazy):
    data = K.all_code_inputs()[name]
    z, r = enc.compress_bytes(data, max_chain=k, flags=D.DMX_ZLIB | (D.DMX_F_LAZY if lazy else 0))
    tok = O.parse_block(data, k, lazy=lazy)
    assert r.nblocks == 1 and np.array_equal(enc.tokens(0), tok)
    bt, costs, lll, ld = O.plan(tok, len(data))
    _, gbt, ghb = enc.blocks(1)
    assert int(gbt[0]) == bt == 2
    ln = enc.code_lengths(0)
    assert ln[:286].tolist() == lll.tolist() and ln[286:].tolist() == ld.tolist()
    if name in K.RLE_NAMES:   # the closed form, no Huffman code in between
        assert ln[:257].tolist() == K.rle_lengths(name) and ln[286:288].tolist() == [1, 1]
    fll, fd = K.histogram(tok)
    check_lengths(fll, ln[:286], 15)
    if fd.any():
        check_lengths(fd, ln[286:], 15)
    h = check_header(z, ln[:286], ln[286:])
    check_lengths(K.cl_histogram(ln[:286], ln[286:]), h["cl_lens"], 7)
    assert int(ghb[0]) == h["end_bit"] - 16
    if name == K.NO_RUNS:   # more than 256 header items: the emission loop's fifth round of 64
        assert len(h["ops"]) > 256
    assert z == O.compress(data, max_chain=k, lazy=lazy)
    assert zlib.decompress(z) == data
    assert D.deflate_decompress(z) == data


@pytest.mark.parametrize("name", OVERFLOW)
def test_overflow_under_split_and_bgzf(enc, name):
    """The same K2 from its other callers: huff_plan per group in the split kernel, BFINAL per member."""
    from test_gpu_bgzf import _want
    data = K.all_code_inputs()[name]
    z, _ = enc.compress_bytes(data, flags=D.DMX_ZLIB | D.DMX_F_SPLIT)
    assert z == O.compress(data, split=True)
    assert zlib.decompress(z) == data and D.deflate_decompress(z) == data
    z, _ = enc.compress_bytes(data, flags=D.DMX_BGZF)
    assert z == _want(data)
    assert gzip.decompress(z) == data


@pytest.mark.parametrize("name", ["fib89", "dfib18"])
def test_overflow_gpu_inflate(enc, name):
    """One indexed GPU inflate of a block whose codes reach 15 bits."""
    data = K.all_code_inputs()[name]
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    out, r = enc.compress_tensor(t, opts=D.Opts(32768, 0, D.DMX_ZLIB, 0))
    assert max(C.max_code_lengths(out.cpu().numpy().tobytes())) == 15
    ix, nb = enc.block_index()
    dec, st = D.inflate_gpu(out, len(data), ix, nb)
    assert st == 0 and dec.cpu().numpy().tobytes() == data


@pytest.mark.parametrize("name", sorted(K.ties()))
def test_type_ties(enc, name):
    data, _ = K.ties()[name]
    z, _ = enc.compress_bytes(data)
    costs = O.plan(O.parse_block(data), len(data))[1]
    _, gbt, _ = enc.blocks(1)
    assert int(gbt[0]) == K.want_btype(costs), costs
    assert z == O.compress(data)
    assert zlib.decompress(z) == data
