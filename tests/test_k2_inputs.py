"""The inputs of tests/k2_inputs.py do what they claim, on the CPU: each witness (a Huffman depth
above the limit by heapq, the run classes, the cost relation of a tie) is stated without
oracle.huff_lengths; then the oracle's plan and stream for the input are held to RFC 1951 and
DESIGN.md §4.1 / §4.3 / §4.4 -- limits, complete codes, no longer code for a larger weight, a
header that spells the lengths the plain run-length way, a stream zlib inflates.
tests/test_gpu_k2_codes.py holds K2 to the same on these blocks."""
import zlib

import numpy as np
import pytest

import deflate_craft as C
import k2_inputs as K
from oracle import oracle as O

CODE_CASES = [(name, k, lazy) for name, ps in K.PARSES.items() for k, lazy in ps]


def check_lengths(freq, lens, limit):
    """DESIGN.md §4.1 on one alphabet: codes for the used symbols only, none above the limit,
    Kraft-complete with two or more codes, and never a longer code for a larger weight."""
    freq, lens = [int(x) for x in freq], [int(x) for x in lens]
    used = [s for s, f in enumerate(freq) if f]
    if len(used) >= 2:
        assert [s for s, n in enumerate(lens) if n] == used
        assert max(lens) <= limit
        assert C.kraft(lens) == 32768
        order = sorted(used, key=lambda s: freq[s])
        for a, b in zip(order, order[1:]):
            assert freq[a] == freq[b] or lens[a] >= lens[b], (a, b)
    else:   # none or one: two codes of length 1 (or none at all)
        assert sorted(n for n in lens if n) in ([], [1, 1])


def check_header(z, lll, ld):
    """The first block's header against RFC 1951 §3.2.7: the lengths, a complete code-length
    code of at most 7 bits, and the plain run-length spelling.  Returns the parsed header."""
    h = C.parse_dynamic_header(z)
    assert h is not None and h["bad"] is None
    a, b = K.trimmed(lll, ld)
    assert h["ll"] == a and h["dd"] == b
    assert max(h["cl_lens"]) <= 7 and C.kraft(h["cl_lens"]) == 32768
    assert h["ops"] == K.cl_ops(a + b)
    return h


def test_every_input_is_one_block_and_listed():
    names = set(K.all_code_inputs())
    assert names == set(K.PARSES) and all(0 < len(d) <= K.B for d in K.all_code_inputs().values())
    assert all(0 < len(d) <= K.B for d, _ in K.ties().values())


@pytest.mark.parametrize("name,k,lazy", CODE_CASES)
def test_witness_and_oracle(name, k, lazy):
    data = K.all_code_inputs()[name]
    tok = O.parse_block(data, k, lazy=lazy)
    assert O.replay(tok) == data
    fll, fd = K.histogram(tok)
    bt, costs, lll, ld = O.plan(tok, len(data))
    assert bt == 2 and costs[2] < min(costs[:2])
    depth = K.huffman_depth(fll), K.huffman_depth(fd), K.huffman_depth(K.cl_histogram(lll, ld))
    if name in K.OVERFLOW_LL:
        assert tok.size == K.B and int(tok.max()) < 256          # no trigram twice: literals only
        assert depth[0] > 15 and int(lll.max()) == 15
    if name == K.SHUFFLE:
        assert depth[0] > 15 and int(lll.max()) == 15 and int((tok >> 9 != 0).sum()) > 20
    if name in K.OVERFLOW_D:
        first = K.FIB_CODES[name]
        assert fd.tolist() == [0] * first + K._fib(30 - first)   # every copy found, at its distance
        assert depth[1] > 15 and int(ld.max()) == 15
    if name in K.overflow_cl():
        assert depth[2] > 7
    if name in K.RLE_NAMES:   # dyadic: the lengths in closed form, and the classes the block owns
        assert tok.size == K.B - 1 and int(tok.max()) < 256
        w = np.bincount(np.frombuffer(data, np.uint8), minlength=256)
        want = [15 - int(x).bit_length() + 1 if x else 0 for x in w] + [15]
        assert all(x == 0 or x & (x - 1) == 0 for x in w.tolist()) and want == K.rle_lengths(name)
        assert lll[:257].tolist() == want and ld.tolist() == [1, 1] + [0] * 28
        assert K.RLE_CLASSES[name] - {"items"} <= K.run_classes(want + [1, 1])
    if name == "cross_hlit":
        a, b = K.trimmed(lll, ld)
        assert a[-1] == b[0] and any(s == 16 and i < len(a) < i + c for s, i, c in K.cl_ops(a + b))
    if name == K.NO_RUNS:      # no run of 4 or more among 259 lengths: one header item each
        a, b = K.trimmed(lll, ld)
        assert len(a + b) >= 250 and max(r for _, _, r in K.runs(a + b)) < 4
    check_lengths(fll, lll, 15)
    if fd.any():
        check_lengths(fd, ld, 15)
    else:
        assert ld.tolist() == [1, 1] + [0] * 28
    z = O.compress(data, max_chain=k, lazy=lazy)
    h = check_header(z, lll, ld)
    check_lengths(K.cl_histogram(lll, ld), h["cl_lens"], 7)
    if name in K.overflow_cl():
        assert max(h["cl_lens"]) == 7
    if name == K.NO_RUNS:      # 4 + HCLEN + these: five rounds of 64 in the emission
        assert len(h["ops"]) > 256
    assert zlib.decompress(z) == data


def test_run_class_table():
    """One table says which block owns which class; together the blocks own every required one."""
    assert set(K.RLE_CLASSES) == set(K.RLE_NAMES) | {"cross_hlit"}
    assert set().union(*K.RLE_CLASSES.values()) == K.RLE_REQUIRED


@pytest.mark.parametrize("name", sorted(K.ties()))
def test_tie_relation(name):
    data, (pair, diff) = K.ties()[name]
    bt, costs, _, _ = O.plan(O.parse_block(data), len(data))
    d, margin = K.tie_relation(costs, pair)
    assert d == diff and margin > 0, costs
    assert costs[0] == 42 + 8 * len(data)
    if name in K.CLOSED_TIES:
        assert costs[1] == 10 + 9 * len(data)
    assert bt == K.want_btype(costs)
    z = O.compress(data)
    assert (z[2] >> 1) & 3 == bt and zlib.decompress(z) == data
