"""The inputs of tests/walk_paths_inputs.py do what they claim, on the CPU: every planted copy is
the token the plant names in the oracle's token streams, at every parse setting
tests/test_gpu_walk_paths.py uses; the plants cover the segment offsets the walk distinguishes;
the periodic blocks have the token counts that pick the one-lane walk and the per-wave
resolution.  Then the fused segment walk (csrc/dmx_walk.h) against a position-by-position walk,
in a stand-alone program under ASan + UBSan (tests/c/walk_model.cpp)."""
import os
import subprocess

import pytest

import walk_paths_inputs as W
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return W.build()


def test_plants_cover_the_shapes(built):
    name, data, plants = built[0]
    assert name == "main" and 2 * W.B < len(data) <= 3 * W.B
    by = {}
    for p in plants:
        by.setdefault(p.kind, []).append(p)
    assert all(p.i % W.SEG == 0 for p in by["lit-run-then-match-at-0"])
    assert all(p.i % W.SEG == 31 for p in by["match-at-31"])
    assert all((p.i + p.greedy[0]) % W.SEG == 0 for p in by["match-ends-on-boundary"])
    assert {p.i % W.SEG for p in by["match-258"] if p.greedy[0] == 258} >= {0, 5, 31}
    for n in (2, 3):   # the first position of a chain at offsets 30 and 31: the chain crosses the boundary
        firsts = {p.i % W.SEG for p in by[f"lazy-chain-{n}"] if p.greedy is not None}
        assert firsts >= {30, 31}
    nb = (len(data) + W.B - 1) // W.B
    for b in range(nb):
        bn = min(W.B, len(data) - b * W.B)
        assert any(p.block == b and p.i + p.greedy[0] == bn for p in by["match-ends-at-bn"])
    assert [len(d) - W.B for _, d, _ in built[1:]] == list(W.LAST_BN)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("k", [7, 16, 0])
def test_oracle_tokens_hold_every_plant(built, k, lazy):
    for name, data, plants in built:
        assert W.find_plants(O.parse(data, max_chain=k, lazy=lazy), plants, lazy) == [], name


@pytest.mark.parametrize("lazy", [False, True])
def test_oracle_tokens_hold_every_plant_with_history(built, lazy):
    for name, data, plants in built:
        assert W.find_plants(O.parse(data, max_chain=7, lazy=lazy, dict=True), plants, lazy) == [], name


def test_whole_segments_of_literals(built):
    """Shape 5: the first segment of every block of the main input, and others, are all literals."""
    _, data, _ = built[0]
    for lazy in (False, True):
        for tok in O.parse(data, max_chain=7, lazy=lazy):
            at = W.tokens_at(tok)
            # (a position that starts no token is not in `at`: 0, not None)
            whole = [s for s in range(200) if all(at.get(W.SEG * s + j, 0) is None for j in range(W.SEG))]
            assert 0 in whole and len(whole) >= 8


def test_periodic_blocks_token_counts():
    """Shape 9: fewer than 1024 tokens (the one-lane walk); shape 10: more (W2 and W3)."""
    for lazy in (False, True):
        few = O.parse(W.periodic_block(0), max_chain=7, lazy=lazy)[0]
        many = O.parse(W.periodic_block(2048), max_chain=7, lazy=lazy)[0]
        assert len(few) < 1024 < 2048 <= len(many)
        at = W.tokens_at(few)
        assert at[W.PERIOD] == (258, W.PERIOD) and sum(1 for v in at.values() if v == (258, W.PERIOD)) >= 126


def test_fused_walk_host_model():
    """tests/c/walk_model.cpp ends with `0 failed checks`: dmx_walk_segment against a sequential
    walk for every literal word with <= 4 runs, random words and lengths, every entry offset,
    every cut by bn, literal bits past bn, and a path word met in a run, at a match and never."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.walk"])
    exe = os.path.join(REPO, "build", "c", "walk_model")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("0 failed checks"), out.stdout
