"""Blocks that sit on the thresholds of the noise check (DMX_F_STORE_CHECK)
and on the edges of its sampling, so that one lost, doubled or phantom sample changes the
verdict.  Seeded numpy only; shared by tests/test_store_check_threshold.py (CPU: the numpy
statement below, the oracle's C and test_store_check's numpy; GPU: K0's per-block decision).

The rule, from §4.7 (bn = block bytes; stored iff bn >= 4096 and all four hold):
  bit    8 |2 ones_k - 4096| <= 4096, ones_k = bytes among the first 4096 with bit k set
  S2     256 S2 <= m^2 + (m^2 >> 4) + 256 m, S2 = sum h[c]^2 over the histogram h of the bytes
         at p = 0 (mod s), s = 8 / 4 / 2 / 1 for bn >= 32768 / 16384 / 8192 / 4096, m = ceil(bn / s)
  q      16 q >= bn, q = the 4-gram starts p <= bn - 4 whose hash x(p) has bits 11..13 clear
  coll   64 coll <= 4 q, coll = q - |{x(p) >> 15 : p sampled}|

`cases()` returns Case records.  tags: "edge" (on the passing side of one bound, or one
attainable step beyond it), "drop" (the verdict flips when the sample `drop` is left out),
"control" (the deciding edit made where it must not count), "phantom" (a zero-padded 4-gram
past the block's end would flip the verdict), "size" (bn < 4096 decides).  In every case the
other inequalities keep the slack of SLACK, so only `stat` decides."""
import collections
import functools

import numpy as np

B = 32768
PLANE = 4096
MUL = 0x9E3779B1
STATS = ("bit", "S2", "q", "coll")
# lhs <= SLACK[stat] * rhs for an inequality that does not decide a case
SLACK = {"bit": 0.75, "S2": 0.98, "q": 0.75, "coll": 0.75}

Case = collections.namedtuple("Case", "name block want stat pos tags drop")


def stride(bn: int) -> int:
    return 8 if bn >= 32768 else 4 if bn >= 16384 else 2 if bn >= 8192 else 1


def hashes(a: np.ndarray) -> np.ndarray:
    """x(p) for p = 0 .. len(a) - 4."""
    w = a.astype(np.uint64)
    w = w[:-3] | w[1:-2] << 8 | w[2:-1] << 16 | w[3:] << 24
    return (w * MUL) & 0xFFFFFFFF


def sampled(a: np.ndarray) -> np.ndarray:
    return (hashes(a) & (7 << 11)) == 0


def stats(block, drop=None, window=PLANE, s=None, pad_tail=False):
    """ones[8], S2, m, q, coll of a block.  drop = ("bit" | "hist" | "gram", p) leaves byte p
    out of the bit-plane count, the sample at p out of the histogram, or the 4-gram that
    starts at p (or at each of an array p) out of the sample.  window, s and pad_tail restate the rule wrongly on purpose
    (another bit-plane window, another stride, 4-grams that run into zero padding): the tests
    use them to show that the cases tell such a statement from the right one."""
    a = np.frombuffer(bytes(block), dtype=np.uint8)
    bn = a.size
    kind, p = drop if drop else (None, -1)
    keep = np.ones(min(window, bn), dtype=bool)
    if kind == "bit" and p < keep.size:
        keep[p] = False
    ones = np.unpackbits(a[:keep.size][keep][:, None], axis=1, bitorder="little").sum(axis=0)
    s = s or stride(bn)
    pos = np.arange(0, bn, s)
    if kind == "hist":
        pos = pos[pos != p]
    h = np.bincount(a[pos], minlength=256).astype(np.int64)
    m = -(-bn // s)
    x = hashes(np.concatenate([a, np.zeros(3, np.uint8)]) if pad_tail else a)
    smp = (x & (7 << 11)) == 0
    if kind == "gram":   # (one start or an array of them)
        p = np.atleast_1d(p)
        smp[p[p < smp.size]] = False
    key = x[smp] >> 15
    q = int(key.size)
    return [int(o) for o in ones], int((h * h).sum()), m, q, q - int(np.unique(key).size)


def sides(st, bn: int) -> dict:
    """Every inequality as (lhs, rhs) of lhs <= rhs."""
    ones, S2, m, q, coll = st
    return {"bit": (max(8 * abs(2 * o - PLANE) for o in ones), PLANE),
            "S2": (256 * S2, m * m + ((m * m) >> 4) + 256 * m),
            "q": (bn, 16 * q),
            "coll": (64 * coll, 4 * q)}


def verdict(st, bn: int, strict=None) -> bool:
    """Stored?  strict names one inequality to state wrongly, with < for <=."""
    if bn < 4096:
        return False
    return all(l < r if k == strict else l <= r for k, (l, r) in sides(st, bn).items())


def slack_ok(st, bn: int, deciding) -> bool:
    return all(l <= SLACK[k] * r for k, (l, r) in sides(st, bn).items() if k != deciding)


def s2_target(m: int) -> int:
    """The largest attainable S2 within the bound: S2 has m's parity (h^2 = h mod 2)."""
    t = (m * m + ((m * m) >> 4) + 256 * m) // 256
    return t if (t - m) % 2 == 0 else t - 1


def _noise(bn: int, seed) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, bn, dtype=np.uint8)


def _far(x: int, others, d: int = 16) -> bool:
    return all(abs(x - o) >= d for o in others)


# ---------------------------------------------------------------------------- q
def _reduce_q(a: np.ndarray, target: int, rng, keep_out=(), unique_only=False) -> None:
    """Single-byte edits (off the histogram's positions where the stride leaves any) that each
    un-sample 4-grams, until q == target.  unique_only: leave coll as it is, by touching only
    4-grams whose bucket no other sampled 4-gram shares."""
    bn, s = a.size, stride(a.size)
    x = hashes(a)
    smp = (x & (7 << 11)) == 0
    q = int(smp.sum())
    cnt = np.bincount((x[smp] >> 15).astype(np.int64), minlength=1 << 17) if unique_only else None
    for _ in range(200000):
        if q == target:
            return
        g = int(np.flatnonzero(smp)[rng.integers(q)])
        j = g + int(rng.integers(3))   # (the fourth byte does not reach the hash bits that sample)
        if (s > 1 and j % s == 0) or not _far(j, keep_out, 8):
            continue
        lo, hi = max(j - 3, 0), min(j + 1, bn - 3)   # the 4-grams lo .. hi - 1 hold byte j
        old = a[j]
        a[j] = rng.integers(256)
        nx = hashes(a[lo:hi + 3])
        new = (nx & (7 << 11)) == 0
        dq = int(new.sum()) - int(smp[lo:hi].sum())
        ok = dq < 0 and q + dq >= target
        if ok and unique_only:   # only lone 4-grams leave, none arrives
            gone = x[lo:hi][smp[lo:hi]] >> 15
            ok = not new.any() and all(cnt[int(k)] == 1 for k in gone)
        if not ok:
            a[j] = old
            continue
        if unique_only:
            for k in x[lo:hi][smp[lo:hi]] >> 15:
                cnt[int(k)] -= 1
        x[lo:hi], smp[lo:hi] = nx, new
        q += dq
    raise RuntimeError(f"q not brought to {target} (bn={bn})")


def _q_floor(bn: int) -> int:
    return -(-bn // 16)   # the smallest q with 16 q >= bn


def _q_pair(bn: int, p: int, seed):
    """(fail, pass): q = ceil(bn / 16) - 1, and the same block with one byte changed so that the
    4-gram at p, and no other, becomes sampled."""
    for attempt in range(8):
        rng = np.random.default_rng([seed, attempt])
        a = _noise(bn, [seed, attempt, 1])
        for v in range(256):   # nothing sampled around p to begin with
            a[p:p + 4] = rng.integers(0, 256, 4)
            lo, hi = max(p - 3, 0), min(p + 4, bn - 3)
            if not sampled(a[lo:hi + 3]).any():
                break
        else:
            continue
        _reduce_q(a, _q_floor(bn) - 1, rng, keep_out=(p, p + 3))
        # byte p: the 4-grams p - 3 .. p hold it (byte p + 3 is no use: a 4-gram's last byte
        # reaches only bits 24..31 of its hash)
        lo = max(p - 3, 0)
        for v in range(256):
            b = a.copy()
            b[p] = v
            new = sampled(b[lo:p + 4])
            if new[-1] and not new[:-1].any():
                sa, sb = stats(a), stats(b)
                if sa[3] == _q_floor(bn) - 1 and sb[3] == _q_floor(bn) and slack_ok(sa, bn, "q") \
                        and slack_ok(sb, bn, "q") and not verdict(sa, bn) and verdict(sb, bn):
                    return a, b
    raise RuntimeError(f"no q pair for bn={bn} p={p}")


def _phantom(bn: int, seed) -> np.ndarray:
    """16 q < bn by one sample, and the last three bytes followed by a zero would be sampled."""
    assert bn % 16
    for attempt in range(8):
        rng = np.random.default_rng([seed, attempt])
        a = _noise(bn, [seed, attempt, 1])
        for _ in range(4096):
            a[bn - 8:] = rng.integers(0, 256, 8)
            pad = sampled(np.concatenate([a[bn - 10:], np.zeros(3, np.uint8)]))   # starts bn - 10 .. bn - 1
            if pad[7] and not pad[:7].any() and not pad[8:].any():
                break
        else:
            continue
        _reduce_q(a, _q_floor(bn) - 1, rng, keep_out=(bn - 8, bn - 1))
        st, sp = stats(a), stats(a, pad_tail=True)
        if st[3] == _q_floor(bn) - 1 and sp[3] == st[3] + 1 and not verdict(st, bn) and verdict(sp, bn) \
                and slack_ok(st, bn, "q"):
            return a
    raise RuntimeError(f"no phantom-tail block for bn={bn}")


# ---------------------------------------------------------------------------- coll
def _plant(a: np.ndarray, dst: int, src: int) -> None:
    a[dst:dst + 4] = a[src:src + 4].copy()


@functools.lru_cache(maxsize=None)
def _coll_base(bn: int, seed: int):
    """Noise with copies of sampled 4-grams planted until coll is a few steps under q / 16."""
    rng = np.random.default_rng([seed, bn])
    a = _noise(bn, [seed, bn, 1])
    for _ in range(4096):
        _, _, _, q, coll = stats(a)
        if 16 * (coll + 4) > q:
            return a.tobytes()
        smp = np.flatnonzero(sampled(a))
        for _ in range(max(1, min(16, (q // 16 - coll - 4) // 2))):
            d, s = int(rng.integers(8, bn - 12)), int(smp[rng.integers(smp.size)])
            if abs(d - s) >= 8:
                _plant(a, d, s)
    raise RuntimeError(f"no coll base for bn={bn}")


def _coll_pair(bn: int, p: int, seed: int, equal: bool = False):
    """(pass, fail): coll = floor(q / 16), and the same block with one more copy of a sampled
    4-gram planted at p, which takes coll one step over its bound: leave that 4-gram out and the
    block passes again.  equal: the passing block has 64 coll == 4 q."""
    base = np.frombuffer(_coll_base(bn, seed), dtype=np.uint8)
    for attempt in range(64):
        rng = np.random.default_rng([seed, bn, p, attempt])
        a = base.copy()
        smp = np.flatnonzero(sampled(a))
        src = int(smp[rng.integers(smp.size)])
        if not _far(src, (p,)):
            continue
        for step in range(64):
            f = a.copy()
            _plant(f, p, src)
            sa, sf = stats(a), stats(f)
            if not verdict(sa, bn):
                break
            if not verdict(sf, bn):
                if equal and sa[3] % 16:
                    try:
                        _reduce_q(a, sa[3] - sa[3] % 16, rng, keep_out=(p, p + 3, src, src + 3), unique_only=True)
                    except RuntimeError:
                        break
                    f = a.copy()
                    _plant(f, p, src)
                    sa, sf = stats(a), stats(f)
                good = (verdict(sa, bn) and not verdict(sf, bn) and sa[4] == sa[3] // 16 and sf[4] == sf[3] // 16 + 1
                        and verdict(stats(f, drop=("gram", p)), bn) and slack_ok(sa, bn, "coll")
                        and slack_ok(sf, bn, "coll") and (not equal or sa[3] % 16 == 0))
                if good:
                    return a, f
                break
            cand = np.flatnonzero(sampled(a))
            d, s = int(rng.integers(8, bn - 12)), int(cand[rng.integers(cand.size)])
            if _far(d, (p, src)) and _far(s, (p,)) and abs(d - s) >= 8:
                _plant(a, d, s)
    raise RuntimeError(f"no coll pair for bn={bn} p={p}")


# ---------------------------------------------------------------------------- S2
def _s2_pair(bn: int, p: int, seed: int):
    """(pass, fail, control): S2 on its largest attainable value within the bound, reached by
    moving sampled bytes (never the one at p) onto more frequent values; the same block with the
    sample at p moved onto an equally frequent value (S2 + 2); and the passing block with that
    edit made one byte further on instead, off the stride (None when s = 1)."""
    s = stride(bn)
    assert p % s == 0
    m, T = -(-bn // s), s2_target(-(-bn // s))
    for attempt in range(8):
        rng = np.random.default_rng([seed, bn, p, attempt])
        a = _noise(bn, [seed, bn, p, attempt, 1])
        h = np.bincount(a[::s], minlength=256).astype(np.int64)
        S2 = int((h * h).sum())
        for _ in range(400000):
            if S2 == T:
                break
            j = int(rng.integers(m)) * s
            u, v = int(a[j]), int(rng.integers(256))
            d = 2 * (h[v] - h[u]) + 2
            if j == p or u == v or not 0 < d <= T - S2:
                continue
            a[j] = v
            h[u] -= 1
            h[v] += 1
            S2 += int(d)
        else:
            continue
        u = int(a[p])
        same = [v for v in range(256) if v != u and h[v] == h[u]]
        if not same:
            continue
        f = a.copy()
        f[p] = same[int(rng.integers(len(same)))]
        c = None
        if s > 1 and p + 1 < bn:
            c = a.copy()
            c[p + 1] = f[p]
        sa, sf = stats(a), stats(f)
        if sa[1] == T and sf[1] == T + 2 and verdict(sa, bn) and not verdict(sf, bn) \
                and verdict(stats(f, drop=("hist", p)), bn) and slack_ok(sa, bn, "S2") and slack_ok(sf, bn, "S2") \
                and (c is None or (verdict(stats(c), bn) and slack_ok(stats(c), bn, "S2"))):
            return a, f, c
    raise RuntimeError(f"no S2 pair for bn={bn} p={p}")


# ---------------------------------------------------------------------------- bit planes
def _bit_pair(k: int, high: bool, off: int, seed: int):
    """(pass, fail): ones_k = 2304 and 2305 (high) or 1792 and 1791, differing in bit k of the
    byte at off."""
    bit = np.uint8(1 << k)
    for attempt in range(8):
        rng = np.random.default_rng([seed, k, int(high), off, attempt])
        a = _noise(B, [seed, k, int(high), off, attempt, 1])
        a[off] = (a[off] & ~bit) if high else (a[off] | bit)
        a[PLANE] &= ~bit   # (the control sets it)
        want = 2304 if high else 1792
        order = rng.permutation(PLANE)
        ones = int(((a[:PLANE] >> k) & 1).sum())
        for j in order:
            if ones == want:
                break
            if j == off:
                continue
            if high and not a[j] & bit:
                a[j] |= bit
                ones += 1
            elif not high and a[j] & bit:
                a[j] &= ~bit
                ones -= 1
        f = a.copy()
        f[off] ^= bit
        sa, sf = stats(a), stats(f)
        if sa[0][k] == want and sf[0][k] == want + (1 if high else -1) and verdict(sa, B) and not verdict(sf, B) \
                and slack_ok(sa, B, "bit") and slack_ok(sf, B, "bit") \
                and all(abs(2 * o - PLANE) <= 256 for i, o in enumerate(sa[0]) if i != k):
            return a, f
    raise RuntimeError(f"no bit-plane pair for k={k} high={high} off={off}")


# ---------------------------------------------------------------------------- the list
# 4-gram starts in a full block: chunk c = p >> 4, lane = c & 63, wave = (c >> 6) & 3, i = c >> 8
def gram_full_positions():
    ps = [0, B - 4]
    ps += [((2 * 256 + 64 + 17) << 4) + r for r in (0, 12, 13, 14, 15)]         # an inner lane (17, wave 1, i = 2)
    ps += [((5 * 256 + 128 + 62) << 4) + 14]                                    # lane 62 into lane 63
    ps += [((i * 256 + w * 64 + 63) << 4) + r for i in range(8) for w in (0, 3) for r in (13, 14, 15)
           if (i, w) != (7, 3)]   # lane 63 into the next wave's chunk (the last chunk has none: B - 4 above)
    return ps


GRAM_GENERAL_BN = (4096, 4099, 8191, 20001, 32767)
HIST_FULL_POSITIONS = (0, B - 8, 4096, 1024, 24)   # first, last, the 4096-byte thread stride, a wave's first chunk, mid-chunk
HIST_BN = (32767, 16384, 16383, 8192, 8191, 4096)
BIT_OFFSETS = (0, 15, 16, 1023, 1024, 4095)
PHANTOM_BN = (4099, 20001)
# every block size among the cases (known without building them, for parametrised tests)
SIZES = (32768, 32767, 20001, 16384, 16383, 8192, 8191, 4099, 4096, 4095)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, a, want, stat, pos, tags, drop=None):
        out.append(Case(name, a.tobytes(), want, stat, pos, frozenset(tags), drop))

    for bn, ps in [(B, gram_full_positions())] + [(bn, [bn - 4]) for bn in GRAM_GENERAL_BN]:
        for n, p in enumerate(ps):
            a, f = _coll_pair(bn, p, 11, equal=(n == 0))
            add(f"coll_{bn}_p{p}_pass", a, True, "coll", p, {"edge"})
            add(f"coll_{bn}_p{p}_fail", f, False, "coll", p, {"edge", "drop"}, ("gram", p))
    for bn, p in [(B, ((3 * 256 + 3 * 64 + 63) << 4) + 14), (4096, 4092), (20001, 19997)]:
        f, a = _q_pair(bn, p, 12)
        add(f"q_{bn}_p{p}_pass", a, True, "q", p, {"edge", "drop"}, ("gram", p))
        add(f"q_{bn}_p{p}_fail", f, False, "q", p, {"edge"})
    for bn in PHANTOM_BN:
        add(f"q_{bn}_phantom", _phantom(bn, 13), False, "q", bn - 3, {"phantom"})
    for bn, ps in [(B, HIST_FULL_POSITIONS)] + [(bn, ((bn - 1) // stride(bn) * stride(bn),) + ((0,) if bn == 16384 else ()))
                                                 for bn in HIST_BN]:
        for p in ps:
            a, f, c = _s2_pair(bn, p, 14)
            add(f"S2_{bn}_p{p}_pass", a, True, "S2", p, {"edge"})
            add(f"S2_{bn}_p{p}_fail", f, False, "S2", p, {"edge", "drop"}, ("hist", p))
            if c is not None and (bn == B or p == 0):
                add(f"S2_{bn}_p{p + 1}_control", c, True, "S2", p + 1, {"control"})
    n = 0
    for k in range(8):
        for high in (True, False):
            off = BIT_OFFSETS[n % len(BIT_OFFSETS)]
            n += 1
            a, f = _bit_pair(k, high, off, 15)
            side = "hi" if high else "lo"
            # high: the failing block has the surplus bit at off; low: the passing block's last needed bit is there
            add(f"bit{k}_{side}_o{off}_pass", a, True, "bit", off, {"edge"} | (set() if high else {"drop"}),
                None if high else ("bit", off))
            add(f"bit{k}_{side}_o{off}_fail", f, False, "bit", off, {"edge"} | ({"drop"} if high else set()),
                ("bit", off) if high else None)
            if high and k in (0, 7):   # the surplus bit just outside the window
                c = a.copy()
                assert not c[PLANE] & (1 << k)
                c[PLANE] |= np.uint8(1 << k)
                add(f"bit{k}_hi_o{PLANE}_control", c, True, "bit", PLANE, {"control"})
            if high and k == 3:        # one byte short of a window: the size decides, whatever the planes say
                add(f"bit{k}_hi_4095_bytes", a[:4095], False, "size", 4095, {"size"})
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def by_size():
    """{bn: [cases]} with passing and failing blocks interleaved as far as they go (a
    phantom-tail block comes last: what follows it in memory is then zero or nothing)."""
    g = {}
    for c in cases():
        g.setdefault(len(c.block), []).append(c)
    for bn, cs in g.items():
        t, f = [c for c in cs if c.want], [c for c in cs if not c.want]
        mix = [c for pr in zip(t, f) for c in pr]
        g[bn] = mix + t[len(f):] + f[len(t):]
        assert all("phantom" not in c.tags for c in g[bn][:-1])
    assert sorted(g) == sorted(SIZES)
    return g
