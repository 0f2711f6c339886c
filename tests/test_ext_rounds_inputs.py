"""The inputs of tests/ext_rounds_inputs.py do what they claim, on the CPU: every planted copy
is a match token of the planted length and distance in the oracle's token streams, at every
parse setting tests/test_gpu_ext_rounds.py uses; no block is stored by the noise check or
deepened by DMX_F_DEEP (either would take the copies off the short-chain search); the plants
cover every length, alignment and block-end gap the extension's rounds distinguish.  Then the
first-mismatch arithmetic of the rounds (csrc/dmx_extbits.h) against a byte loop, in a
stand-alone program under ASan + UBSan (tests/c/ext_rounds_model.cpp)."""
import os
import subprocess

import pytest

import ext_rounds_inputs as X
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return X.build()


def test_plants_cover_the_cases(built):
    data, plants = built
    assert len(data) <= 8 * X.B
    lens = [p for p in plants if p.kind == "len"]
    # every length at each of the 16 (i mod 4, q mod 4); 8..12 put the mismatch in each byte of a word
    for ln in X.LENGTHS:
        got = {(p.i % 4, (p.i - p.dist) % 4) for p in lens if p.length == min(ln, X.MAXLEN)}
        assert len(got) == 16, ln
    nb = (len(data) + X.B - 1) // X.B
    ends = sorted((min(X.B, len(data) - p.block * X.B) - p.i) for p in plants if p.kind == "end")
    assert ends == sorted(X.END_GAPS)
    assert any(p.kind == "end" and p.block == nb - 1 for p in plants) and len(data) % X.B == X.SHORT_LAST
    for kind in ("LLL", "LMM", "LLF", "NLL"):
        assert sorted(p.length for p in plants if p.kind == kind) == sorted(
            L + (kind != "LLL") + 39 * (kind == "LLF") for L in X.TRIPLE_L)
    assert sum(p.hist for p in plants) >= 16


def test_first_entries_of_s(built):
    """The "first" plants are among the first K entries of S: fewer than 6 earlier positions of
    their block hash to their bucket or a lower one."""
    data, plants = built
    first = [p for p in plants if p.kind == "first"]
    assert len(first) == 2
    for p in first:
        blk = data[p.block * X.B:(p.block + 1) * X.B]
        hb = X.bucket(*blk[p.i:p.i + 3])
        assert hb == 0
        k = sum(1 for x in range(len(blk) - 2) if X.bucket(*blk[x:x + 3]) == 0 and x < p.i)
        assert 1 <= k < 6, k


def test_blocks_stay_on_the_short_chain_search(built):
    data, _ = built
    for o in range(0, len(data), X.B):
        blk = data[o:o + X.B]
        assert not O.store_check(blk)
        for k in (6, 7, 8):
            assert O.block_chain(blk, k) == k


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("k", [4, 6, 7, 8, 16, 0])
def test_oracle_tokens_hold_every_plant(built, k, lazy):
    data, plants = built
    assert X.find_plants(O.parse(data, max_chain=k, lazy=lazy), plants, False) == []


@pytest.mark.parametrize("lazy", [False, True])
def test_oracle_tokens_hold_the_history_plants(built, lazy):
    data, plants = built
    assert X.find_plants(O.parse(data, max_chain=7, lazy=lazy, dict=True), plants, True) == []


def test_first_mismatch_formula_host_model():
    """tests/c/ext_rounds_model.cpp ends with `0 failed checks`: dmx_first_diff_bit against a
    byte loop for every mismatch position, every value of the differing byte's low and high
    bit, and both alignments, W = 6 and 8."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.ext_rounds"])
    exe = os.path.join(REPO, "build", "c", "ext_rounds_model")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("0 failed checks"), out.stdout
