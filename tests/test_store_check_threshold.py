"""The noise check (DMX_F_STORE_CHECK) on its four thresholds and at the edges of
its sampling: blocks from tests/store_check_threshold_inputs.py whose verdict hangs on one
sample (a 4-gram that straddles two chunks, lanes or waves, the last 4-gram of a short block,
the first and last histogram sample under every stride, one bit of a plane's window).

CPU: the generator's numpy statement, the oracle's C and test_store_check's numpy agree on every
case; the cases sit where their names say; every class of position is there; and restating
the rule wrongly in the ways a kernel could be wrong changes at least one verdict.
GPU (-m gpu): K0's decision per block (ntok == 0 exactly where the rule stores) under every
route to it -- the default launch, the work-list kernel (SPEC), no work lists, and the general
path by an input shifted off 16-byte alignment -- with the stream equal to the oracle's."""
import functools
import zlib

import numpy as np
import pytest

import deflate_compression_amd as D
from oracle import oracle as O
from tests import store_check_threshold_inputs as G
from tests.store_check_threshold_inputs import B, PLANE, stats, verdict
from tests.test_store_check import np_store_check


@pytest.fixture(scope="module")
def CASES():
    return G.cases()


def _bn(c):
    return len(c.block)


def _chunk(p):
    """(lane, wave, i, p mod 16) of a 4-gram start in a full block (K0's register layout)."""
    c = p >> 4
    return c & 63, (c >> 6) & 3, c >> 8, p & 15


def _diff(c, d):
    """The offsets at which two cases' blocks differ."""
    return np.flatnonzero(np.frombuffer(c.block, np.uint8) != np.frombuffer(d.block, np.uint8)).tolist()


def test_three_statements_agree_with_the_expected_verdict(CASES):
    for c in CASES:
        assert verdict(stats(c.block), _bn(c)) == c.want, c.name
        assert O.store_check(c.block) == c.want, c.name
        assert np_store_check(c.block) == c.want, c.name


def test_only_the_named_statistic_decides(CASES):
    for c in CASES:
        if c.stat == "size":
            continue
        sd = G.sides(stats(c.block), _bn(c))
        for k, (l, r) in sd.items():
            if k != c.stat:
                assert l <= G.SLACK[k] * r, (c.name, k, l, r)
            elif "edge" in c.tags:
                assert (l <= r) == c.want, (c.name, k, l, r)


def test_edges_are_one_step_apart(CASES):
    """The passing block on the bound where parity allows (else on the closest value), the
    failing one a single attainable step beyond."""
    seen = set()
    for c in CASES:
        if "edge" not in c.tags:
            continue
        ones, S2, m, q, coll = stats(c.block)
        bn = _bn(c)
        if c.stat == "bit":
            hit = [(k, o) for k, o in enumerate(ones) if o in ((2304, 1792) if c.want else (2305, 1791))]
            assert len(hit) == 1, c.name
            seen.add(("bit",) + hit[0])
        elif c.stat == "S2":
            assert m == -(-bn // G.stride(bn)) and S2 == G.s2_target(m) + (0 if c.want else 2), c.name
            assert 256 * (G.s2_target(m) + 2) > m * m + ((m * m) >> 4) + 256 * m
            seen.add(("S2", bn, c.want, 256 * S2 == m * m + ((m * m) >> 4) + 256 * m))
        elif c.stat == "q":
            assert q == -(-bn // 16) - (0 if c.want else 1), c.name
            seen.add(("q", bn, c.want, 16 * q == bn))
        else:
            assert coll == q // 16 + (0 if c.want else 1), c.name
            seen.add(("coll", bn, c.want, 16 * coll == q))
    for k in range(8):
        assert {("bit", k, o) for o in (2304, 2305, 1792, 1791)} <= seen, k
    # equality itself where it can be met: S2 at m = 4096, q at a multiple of 16, coll at q = 16 coll
    assert ("S2", B, True, True) in seen and ("q", B, True, True) in seen and ("q", 4096, True, True) in seen
    assert any(s[0] == "coll" and s[2] and s[3] for s in seen)


def test_drop_sensitive_cases_flip(CASES):
    n = 0
    for c in CASES:
        if "drop" not in c.tags:
            assert c.drop is None, c.name
            continue
        assert c.drop[1] == c.pos, c.name
        assert verdict(stats(c.block, drop=c.drop), _bn(c)) != c.want, c.name
        n += 1
    assert n >= 80


def test_controls_and_phantom_tail(CASES):
    by = {c.name: c for c in CASES}
    for c in CASES:
        if "control" in c.tags:   # the deciding edit, made where it does not count
            assert c.want
            if c.stat == "S2":
                p = c.pos - 1
                f = by[f"S2_{_bn(c)}_p{p}_fail"]
                assert c.pos % G.stride(_bn(c)) == 1 and c.block[c.pos] == f.block[p]
                assert _diff(c, by[f"S2_{_bn(c)}_p{p}_pass"]) in ([c.pos], [])
            else:
                a = next(x for x in CASES if x.name.startswith(c.name.split("_o")[0] + "_o") and x.name.endswith("_pass"))
                assert c.pos == PLANE and _diff(c, a) == [PLANE]
        if "phantom" in c.tags:
            bn = _bn(c)
            assert bn % 16 and not c.want and c.pos == bn - 3
            st, sp = stats(c.block), stats(c.block, pad_tail=True)
            assert sp[3] == st[3] + 1 and 16 * st[3] < bn <= 16 * sp[3]
            assert verdict(sp, bn)
        if "size" in c.tags:
            assert _bn(c) == 4095 and not c.want
            assert verdict(stats(c.block + b"\x80"), 4096)   # the same planes pass in a block of 4096


def test_every_class_is_present(CASES):
    drop = [c for c in CASES if "drop" in c.tags]
    # 4-gram starts, full path
    full = {_chunk(c.pos) for c in drop if c.stat == "coll" and _bn(c) == B}
    pos = {c.pos for c in drop if c.stat == "coll" and _bn(c) == B}
    assert {0, B - 4} <= pos
    for r in (0, 12, 13, 14, 15):
        assert any(lane < 62 and rr == r for lane, _, _, rr in full), r
    assert any(lane == 62 and rr >= 13 for lane, _, _, rr in full)
    for i in range(8):
        for w in (0, 3):
            for r in (13, 14, 15):
                if (i, w) != (7, 3):   # (the block's last chunk: its last 4-gram is B - 4)
                    assert (63, w, i, r) in full, (i, w, r)
    assert any(c.stat == "q" and _bn(c) == B and _chunk(c.pos)[0] == 63 and c.pos & 15 >= 13 for c in drop)
    # 4-gram starts, general path: the last one of a short block, and the phantom after it
    assert {_bn(c) for c in drop if c.stat == "coll" and c.pos == _bn(c) - 4} >= {4096, 4099, 8191, 20001, 32767}
    assert any("phantom" in c.tags for c in CASES)
    # histogram samples
    hp = {c.pos for c in drop if c.stat == "S2" and _bn(c) == B}
    assert {0, B - 8} <= hp and any(p and p % 4096 == 0 for p in hp) and any(p % 4096 and p % 16 == 0 for p in hp)
    assert any(c.stat == "S2" and "control" in c.tags and _bn(c) == B for c in CASES)
    for bn in (32768, 32767, 16384, 16383, 8192, 8191, 4096):
        s = G.stride(bn)
        assert any(c.stat == "S2" and _bn(c) == bn and c.pos == (bn - 1) // s * s for c in drop), bn
    assert [G.stride(bn) for bn in (32768, 32767, 16384, 16383, 8192, 8191, 4096)] == [8, 4, 4, 2, 2, 1, 1]
    # bit planes
    assert {c.pos for c in drop if c.stat == "bit"} == {0, 15, 16, 1023, 1024, 4095}
    assert any(c.stat == "bit" and "control" in c.tags and c.pos == PLANE for c in CASES)
    assert any("size" in c.tags for c in CASES)
    # both verdicts in each family and for each statistic
    for tag in ("edge", "drop"):
        assert {c.want for c in CASES if tag in c.tags} == {True, False}, tag
    for st in G.STATS:
        assert {c.want for c in CASES if c.stat == st} == {True, False}, st


def test_packing_by_size(CASES):
    """The GPU inputs: every case once, one block size per input, the verdicts interleaved."""
    g = G.by_size()
    assert tuple(sorted(g, reverse=True)) == G.SIZES
    assert sorted(c.name for cs in g.values() for c in cs) == sorted(c.name for c in CASES)
    for bn, cs in g.items():
        assert all(_bn(c) == bn for c in cs)
    want = [c.want for c in g[B]]
    assert sum(a != b for a, b in zip(want, want[1:])) >= len(want) // 2


def _straddles63(bn):
    p = np.arange(bn - 3)
    return p[((p >> 4) & 63 == 63) & (p & 15 >= 13)]


MUTANTS = {
    # the statement, wrong in one way a kernel could be wrong
    "4-grams that straddle lane 63 lost": lambda blk, bn: verdict(stats(blk, drop=("gram", _straddles63(bn))), bn),
    "zero-padded tail 4-grams counted": lambda blk, bn: verdict(stats(blk, pad_tail=True), bn),
    "stride 8 from 16384 bytes": lambda blk, bn: verdict(stats(blk, s=8 if bn >= 16384 else None), bn),
    "< in the bit-plane test": lambda blk, bn: verdict(stats(blk), bn, strict="bit"),
    "< in the S2 test": lambda blk, bn: verdict(stats(blk), bn, strict="S2"),
    "< in the q test": lambda blk, bn: verdict(stats(blk), bn, strict="q"),
    "< in the coll test": lambda blk, bn: verdict(stats(blk), bn, strict="coll"),
    "bit-plane window of 4095 bytes": lambda blk, bn: verdict(stats(blk, window=4095), bn),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_cases_tell_a_wrong_statement(CASES, name):
    wrong = [c.name for c in CASES if MUTANTS[name](c.block, _bn(c)) != c.want]
    print(f"{name}: {len(wrong)} of {len(CASES)} cases disagree, e.g. {wrong[:3]}")
    assert wrong


# ---------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu
K = 4


@functools.lru_cache(maxsize=None)
def _expected(bn):
    """(input, oracle stream, token count per block that the check leaves to the parse)."""
    cs = G.by_size()[bn]
    data = b"".join(c.block for c in cs)
    ntok = [None if c.want else len(O.parse_block(c.block, max_chain=K)) for c in cs]
    return data, O.compress(data, sw=bn, max_chain=K, store_check=True), ntok


@pytest.fixture(scope="module")
def enc():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = D.Encoder(0, 8 << 20)
    yield e
    e.close()


ROUTES = {"default": (None, 0), "worklist_list": ("list", 0), "worklist_off": ("0", 0),
          "shift1": (None, 1), "shift8": (None, 8)}


@gpu
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("bn", G.SIZES)
def test_gpu_decision_per_block(enc, bn, route):
    """One case per sw = bn block.  shift: the input tensor starts 1 or 8 bytes past a 16-byte
    boundary, so full blocks take K0's general path too."""
    import torch
    cs = G.by_size()[bn]
    data, want, ntok = _expected(bn)
    shape, shift = ROUTES[route]
    buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    buf[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    t = buf[shift:shift + len(data)]
    assert t.data_ptr() % 16 == shift
    enc.set_hook("worklist", shape)
    try:
        z, r = enc.compress_tensor(t, opts=D.Opts(bn, K, D.DMX_ZLIB | D.DMX_F_STORE_CHECK, 0))
    finally:
        enc.set_hook("worklist", None)
    assert r.status == 0 and r.nblocks == len(cs)
    nt, bt, hb = enc.blocks(len(cs))
    assert len(nt) == len(cs)
    for b, c in enumerate(cs):
        if c.want:
            assert nt[b] == 0 and bt[b] == 0 and hb[b] == 3, (c.name, b, int(nt[b]), int(bt[b]), int(hb[b]))
        else:
            assert nt[b] == ntok[b] and ntok[b] > 0, (c.name, b, int(nt[b]), ntok[b])
    z = z.cpu().numpy().tobytes()
    assert z == want
    assert zlib.decompress(z) == data
