"""The counting sort's slice map (csrc/dmx_sort_slices.h) on the CPU: slice
s = 4g + r is positions [2048 s, 2048 s + 2048), belongs to group g, ranks in round r and is run
by wave 4g + ((g + r) & 3).  tests/c/sort_slices.cpp prints the header's functions as the host
compiles them; the kernel compiles the same text."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.slices"])
    out = subprocess.run([os.path.join(REPO, "build", "c", "sort_slices")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(16))
    return {"wave_of_slice": [r[1] for r in rows], "slice_of_wave": [r[2] for r in rows],
            "group": [r[3] for r in rows], "round": [r[4] for r in rows]}


def test_bijection(table):
    assert sorted(table["wave_of_slice"]) == list(range(16))
    assert sorted(table["slice_of_wave"]) == list(range(16))
    for s in range(16):
        assert table["slice_of_wave"][table["wave_of_slice"][s]] == s


def test_slices_stay_in_their_group(table):
    """A group is four waves w >> 2 and the position range [8192 g, 8192 g + 8192)."""
    for s in range(16):
        assert table["group"][s] == s >> 2
        assert table["wave_of_slice"][s] >> 2 == s >> 2


def test_a_rounds_waves_have_four_different_w_mod_4(table):
    for r in range(4):
        waves = [table["wave_of_slice"][s] for s in range(16) if table["round"][s] == r]
        assert len(waves) == 4
        assert sorted(w & 3 for w in waves) == [0, 1, 2, 3]
        assert sorted(w >> 2 for w in waves) == [0, 1, 2, 3]   # one of each group


def test_a_groups_rounds_visit_its_slices_in_position_order(table):
    for g in range(4):
        by_round = sorted((table["round"][s], s) for s in range(16) if table["group"][s] == g)
        assert [r for r, _ in by_round] == [0, 1, 2, 3]
        assert [s for _, s in by_round] == [4 * g, 4 * g + 1, 4 * g + 2, 4 * g + 3]
