"""DMX_F_DEEP at its threshold, on the CPU: the two blocks of tests/deep_threshold_inputs.py
have D = 1023 and D = 1024 distinct sampled buckets of 4 096 samples, so the rule 4 D < samples
calls the first deep and the second not.  Pins the inputs that tests/test_gpu_k1_housekeeping.py
gives the match kernel, where the statistic comes from the counting sort's own hashes."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.deep_threshold_inputs import SAMPLES, B, distinct_buckets, pair

DEEP_K = 32   # DMX_DEEP_CHAIN


def test_pair_sits_on_the_threshold():
    deep, shallow = pair()
    assert len(deep) == len(shallow) == B
    dd = distinct_buckets(np.frombuffer(deep, dtype=np.uint8))
    ds = distinct_buckets(np.frombuffer(shallow, dtype=np.uint8))
    assert (dd, ds) == (1023, 1024)
    assert 4 * dd == SAMPLES - 4 and 4 * ds == SAMPLES


@pytest.mark.parametrize("k", [1, 7, 8])
def test_oracle_verdict_on_the_pair(k):
    deep, shallow = pair()
    assert O.block_chain(deep, k) == DEEP_K
    assert O.block_chain(shallow, k) == k


def test_oracle_verdict_follows_the_depth_setting():
    """Above KD = 32 the kernel asks block_chain before the sort: the same verdicts at depth 48."""
    deep, shallow = pair()
    O.set_deep_chain(48)
    try:
        assert O.block_chain(deep, 7) == 48
        assert O.block_chain(shallow, 7) == 7
    finally:
        O.set_deep_chain(0)


def test_parses_differ_only_by_depth():
    deep, shallow = pair()
    assert np.array_equal(O.parse_block(deep, 7, lazy=True, deep=True), O.parse_block(deep, DEEP_K, lazy=True))
    assert np.array_equal(O.parse_block(shallow, 7, lazy=True, deep=True), O.parse_block(shallow, 7, lazy=True))
