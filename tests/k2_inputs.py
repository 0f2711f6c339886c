"""Single blocks that drive the parts of K2 (dmx_huff_kernel) that
natural inputs leave alone: codes longer than their limit in each of the three alphabets (the
overflow redistribution and the length assignment after it), every class of the closed-form
run-length coding of the code lengths, and the two tie rules of the block type.

    overflow_ll()   {name: block}   lit/len Huffman depth above 15 (Fibonacci bottom + fillers)
    overflow_d()    {name: block}   distance Huffman depth above 15 (Fibonacci over the distance codes)
    overflow_cl()   {name: block}   code-length Huffman depth above 7
    rle_blocks()    {name: block}   dyadic, literal-only: the lengths in closed form (rle_lengths)
    RLE_CLASSES     {name: the run classes the block owns}; their union is RLE_REQUIRED
    cross_hlit()    a block whose last lit/len length starts a run that goes on in the distance lengths
    ties()          {name: (block, relation of (stored, fixed, dynamic))}

Witnesses, stated without oracle.huff_lengths: histogram (tokens -> the two frequency tables),
huffman_depth (heapq), cl_histogram (deflate_craft.cl_rle over the trimmed lengths), runs.

Shared by tests/test_k2_inputs.py (the witnesses and the oracle, no GPU) and
tests/test_gpu_k2_codes.py (the kernel).  Deterministic: fixed seeds, numpy + stdlib only; every
block is built once per process.
"""
import bisect
import functools
import heapq

import numpy as np

import deflate_craft as C

B = 32768
EOB = 256


# ------------------------------------------------------------------------------------------
# Witnesses
# ------------------------------------------------------------------------------------------
def histogram(tok):
    """(lit/len counts[286], distance counts[30]) of a token array (t = byte, or dist << 9 | len),
    the end-of-block symbol counted once."""
    t = np.asarray(tok, dtype=np.int64)
    d, l = t >> 9, t & 0x1FF
    fll = np.bincount(t[d == 0] & 0xFF, minlength=286)
    m = d != 0
    fll += np.bincount(257 + np.searchsorted(C.LBASE, l[m], side="right") - 1, minlength=286)
    fd = np.bincount(np.searchsorted(C.DBASE, d[m], side="right") - 1, minlength=30)
    fll[EOB] += 1
    return fll, fd


def huffman_depth(freq):
    """Longest code of an unconstrained Huffman code of the non-zero counts.  Equal weights merge
    the shallower subtree first, so no other tie order gives a flatter tree at that step."""
    h = [(int(f), 0, s) for s, f in enumerate(freq) if f]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    k = len(freq)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1, k))
        k += 1
    return h[0][1]


def trimmed(lll, ld):
    """The header's concatenated length list: lit/len lengths to HLIT (>= 257), distance
    lengths to HDIST (>= 1)."""
    lll, ld = [int(x) for x in lll], [int(x) for x in ld]
    hl, hd = 286, 30
    while hl > 257 and lll[hl - 1] == 0:
        hl -= 1
    while hd > 1 and ld[hd - 1] == 0:
        hd -= 1
    return lll[:hl], ld[:hd]


def cl_histogram(lll, ld):
    """Counts of the 19 code-length symbols in the plain run-length spelling of the header."""
    a, b = trimmed(lll, ld)
    f = [0] * 19
    for s in C.cl_rle(a + b):
        f[s if isinstance(s, int) else s[0]] += 1
    return f


def cl_ops(lens):
    """cl_rle(lens) in parse_dynamic_header's form: [(symbol, first index, count)]."""
    out, i = [], 0
    for s in C.cl_rle(lens):
        n = 1 if isinstance(s, int) else (3 if s[0] != 18 else 11) + s[1]
        out.append((s if isinstance(s, int) else s[0], i, n))
        i += n
    assert i == len(lens)
    return out


def runs(lens):
    """[(value, first index, run length)] of a list of lengths."""
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        out.append((lens[i], i, j - i))
        i = j
    return out


def run_classes(lens):
    """The classes of DESIGN.md §4.3 a length list contains: ("z" | "n", R) for every zero /
    non-zero run, ("zx" | "nx", k) for a run that holds indices k - 1 and k, k a multiple of 64."""
    out = set()
    for v, i, r in runs(lens):
        out.add(("n" if v else "z", r))
        for k in (64, 128, 192, 256):
            if i < k < i + r:
                out.add(("nx" if v else "zx", k))
    return out


# ------------------------------------------------------------------------------------------
# Building blocks
# ------------------------------------------------------------------------------------------
def _tri(a, b, c):
    return (a << 16) | (b << 8) | c


def _bucket(a, b, c):
    """The match search's 13-bit hash of a trigram."""
    return (((a | (b << 8) | (c << 16)) * 0x9E3779B1) & 0xFFFFFFFF) >> 19


def _repeat_free(pool):
    """The multiset `pool` (a shuffled list of byte values) in an order in which no trigram
    occurs twice: the next value is the last one in the pool that completes a new trigram.
    Values for which the end of the block has no place left go into the first earlier gap
    where the three trigrams they make are new."""
    pool = list(pool)
    out, seen = [], set()
    while pool:
        for j in range(len(pool) - 1, -1, -1):
            x = pool[j]
            if len(out) < 2 or _tri(out[-2], out[-1], x) not in seen:
                break
        else:
            break
        pool.pop(j)
        if len(out) >= 2:
            seen.add(_tri(out[-2], out[-1], x))
        out.append(x)
    i = 2
    for x in pool:
        while True:
            assert i + 1 < len(out), "no gap left that takes the value"
            a, b, c, d = out[i - 2:i + 2]
            new = {_tri(a, b, x), _tri(b, x, c), _tri(x, c, d)}
            if len(new) == 3 and not new & seen:
                break
            i += 1
        seen -= {_tri(a, b, c), _tri(b, c, d)}
        seen |= new
        out.insert(i, x)
        i += 3
    return bytes(out)


def _repeat_free_random(n, rng):
    """n random bytes, each drawn again while it completes a trigram already seen."""
    out, seen = [], set()
    draw = iter(())
    while len(out) < n:
        x = next(draw, None)
        if x is None:
            draw = iter(rng.integers(0, 256, 4096).tolist())
            continue
        if len(out) >= 2:
            t = _tri(out[-2], out[-1], x)
            if t in seen:
                continue
            seen.add(t)
        out.append(x)
    return out, seen


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


# ------------------------------------------------------------------------------------------
# Lit/len codes over 15 bits
# ------------------------------------------------------------------------------------------
def _fib_multiset(top, fillers, seed):
    """Literal counts: the Fibonacci chain 1, 2, 3, 5 ... top (the end-of-block symbol is the
    chain's other 1) on random byte values, the rest of the block spread over `fillers` more
    values of nearly equal weight.  Returns the shuffled multiset."""
    rng = np.random.default_rng(seed)
    chain = [f for f in _fib(40)[1:] if f <= top]
    syms = rng.permutation(256)[:len(chain) + fillers].tolist()
    rest = B - sum(chain)
    w = chain + [rest // fillers + (1 if k < rest % fillers else 0) for k in range(fillers)]
    pool = np.repeat(np.array(syms, dtype=np.uint8), w)
    assert pool.size == B
    return rng.permutation(pool).tolist()


OVERFLOW_LL = {"fib89": (89, 200, 11), "fib144": (144, 190, 12), "fib233": (233, 170, 13)}
LITERAL_ONLY = tuple(OVERFLOW_LL)        # no trigram twice: 32768 literals under every parse
SHUFFLE = "fib89_shuffle"                # the same multiset as fib89, plainly shuffled: some matches


@functools.lru_cache(maxsize=None)
def overflow_ll():
    out = {name: _repeat_free(_fib_multiset(*spec)) for name, spec in OVERFLOW_LL.items()}
    out[SHUFFLE] = bytes(_fib_multiset(*OVERFLOW_LL["fib89"]))
    return out


# ------------------------------------------------------------------------------------------
# Distance codes over 15 bits
# ------------------------------------------------------------------------------------------
def _fib_distances(base_len, first_code, seed):
    """A repeat-free random base, then 3-byte copies of distinct base positions whose distances
    give the distance codes first_code .. 29 the counts 1, 1, 2, 3, 5 ...  The copies come in
    ascending code order (short distances while the base is near), each at the smallest distance
    of its code that is free and leaves the parse no choice: the copied trigram occurs once
    before, the match cannot extend, and the two trigrams across the seam are new.  A source
    is also passed over when six positions after it share its hash bucket, so the
    bounded search (max_chain 8) finds the same copies but for a few."""
    rng = np.random.default_rng(seed)
    data, seen = _repeat_free_random(base_len, rng)
    chain = {}         # bucket -> positions, ascending
    for q in range(base_len - 2):
        chain.setdefault(_bucket(*data[q:q + 3]), []).append(q)
    seam = set()       # trigrams made across the copies' seams: not in the base
    used = set()
    prev = None        # the previous copy's source
    for code, count in zip(range(first_code, 30), _fib(30 - first_code)):
        lo, hi = C.DBASE[code], C.DBASE[code] + (1 << C.DEXT[code]) - 1
        for _ in range(count):
            p = len(data)
            for d in range(max(lo, p - (base_len - 4)), min(hi, p) + 1):
                s = p - d
                if s in used:
                    continue
                a, b, c = data[s:s + 3]
                if _tri(a, b, c) in seam:
                    continue
                if prev is not None and data[prev + 3] == a:
                    continue
                t1, t2 = _tri(data[-2], data[-1], a), _tri(data[-1], a, b)
                if t1 in seen or t2 in seen or t1 == t2:
                    continue
                if len(chain[_bucket(a, b, c)]) - bisect.bisect_right(chain[_bucket(a, b, c)], s) >= 6:
                    continue
                break
            else:
                raise AssertionError(f"no free distance for code {code}")
            used.add(s)
            seen.update((t1, t2))
            seam.update((t1, t2))
            data += [a, b, c]
            for q in (p - 2, p - 1, p):
                chain.setdefault(_bucket(*data[q:q + 3]), []).append(q)
            prev = s
    assert len(data) <= B
    return bytes(data)


OVERFLOW_D = {"dfib17": (20000, 13, 21), "dfib18": (12400, 12, 22)}
FIB_CODES = {"dfib17": 13, "dfib18": 12}


@functools.lru_cache(maxsize=None)
def overflow_d():
    return {name: _fib_distances(*spec) for name, spec in OVERFLOW_D.items()}


# ------------------------------------------------------------------------------------------
# Code-length codes over 7 bits
# ------------------------------------------------------------------------------------------
# Plain shuffles of the Fibonacci multisets: the few matches and the overflow repair leave a
# header whose 19-symbol histogram has a Huffman depth of 8 or 9.  The seeds were found by a
# search over 100..159 with cl_histogram / huffman_depth as the witness; fib144 is one more.
OVERFLOW_CL = {SHUFFLE: OVERFLOW_LL["fib89"], "fib89_shuffle102": (89, 200, 102), "fib89_shuffle130": (89, 200, 130),
               "fib144_shuffle120": (144, 190, 120)}


@functools.lru_cache(maxsize=None)
def overflow_cl():
    out = {name: bytes(_fib_multiset(*spec)) for name, spec in OVERFLOW_CL.items()}
    out["fib144"] = overflow_ll()["fib144"]
    return out


# ------------------------------------------------------------------------------------------
# A run of equal lengths across HLIT | HDIST
# ------------------------------------------------------------------------------------------
def _runny(seed):
    """Short runs of a few byte values (the family the seeds below were searched in)."""
    rng = np.random.default_rng(seed)
    n, k = int(rng.integers(40, 400)), int(rng.integers(2, 6))
    parts = []
    while sum(map(len, parts)) < n:
        parts.append(bytes([int(rng.integers(0, k))]) * int(rng.integers(1, 8)))
    return b"".join(parts)[:n]


CROSS_HLIT_SEED = 555   # lengths ... 3 3 3 | 3 ...: the repeat (16) starts in the lit/len lengths and ends behind HLIT


@functools.lru_cache(maxsize=None)
def cross_hlit():
    return _runny(CROSS_HLIT_SEED)


# ------------------------------------------------------------------------------------------
# Block type ties: fixed <= dynamic gives fixed, stored < best gives stored
# ------------------------------------------------------------------------------------------
# name: (seed, lowest n, highest n + 1, lowest byte, highest byte + 1, which two costs, first - second);
# the third cost is above both.  Found by a search over seeds 0..2999 with oracle.plan.
TIES = {
    "fix_eq_dyn": (54, 30, 60, 0, 26, "fd", 0),
    "fix_below_dyn": (113, 30, 60, 0, 26, "fd", -1),
    "fix_above_dyn": (126, 30, 60, 0, 26, "fd", 1),
    "sto_eq_dyn": (17, 250, 300, 117, 256, "sd", 0),
    "sto_below_dyn": (8, 250, 300, 117, 256, "sd", -1),
    "sto_above_dyn": (12, 250, 300, 117, 256, "sd", 1),
    "sto_eq_fix": (1, 30, 35, 183, 256, "sf", 0),
    "sto_below_fix": (4, 30, 35, 183, 256, "sf", -1),
    "sto_above_fix": (21, 30, 35, 183, 256, "sf", 1),
}
# the closed form: n distinct bytes >= 144 cost 10 + 9 n fixed and 42 + 8 n stored
CLOSED_TIES = {"distinct32": (32, "sf", 0), "distinct33": (33, "sd", 0)}


@functools.lru_cache(maxsize=None)
def ties():
    """{name: (block, (pair, difference))}"""
    out = {}
    for name, (seed, n0, n1, lo, hi, pair, diff) in TIES.items():
        rng = np.random.default_rng(seed)
        n = int(rng.integers(n0, n1))
        out[name] = (rng.integers(lo, hi, n, dtype=np.uint8).tobytes(), (pair, diff))
    for name, (n, pair, diff) in CLOSED_TIES.items():
        out[name] = (bytes(range(144, 144 + n)), (pair, diff))
    return out


def tie_relation(costs, pair):
    """(first - second of the pair, the third cost's margin above both) for (stored, fixed, dynamic)."""
    s, f, d = costs
    a, b, c = {"fd": (f, d, s), "sd": (s, d, f), "sf": (s, f, d)}[pair]
    return a - b, c - max(a, b)


def want_btype(costs):
    """DESIGN.md §4.4 stated on the three costs: dynamic unless fixed <= dynamic; stored only if below both."""
    s, f, d = costs
    bt, best = (1, f) if f <= d else (2, d)
    return 0 if s < best else bt


# ------------------------------------------------------------------------------------------
# Run-length classes on dyadic blocks
# ------------------------------------------------------------------------------------------
# Literal-only, repeat-free blocks of 32767 bytes whose byte counts are powers of two: with the
# end-of-block symbol the weights sum to 2^15, so the lit/len lengths are 15 - log2(count) in
# closed form -- no Huffman code is needed to state them.  name: (shuffle seed, [(length, run)]
# over the literals 0..255); the end-of-block length is 15, the distance lengths are 1 1.
RLE_BLOCKS = {
    "small": (5, [
        (9, 1), (0, 1), (10, 2), (0, 2), (7, 3), (0, 3), (8, 4), (0, 10), (14, 5), (0, 11), (11, 6), (0, 12),
        (9, 4), (6, 7), (7, 8), (5, 9), (10, 10), (8, 11), (5, 13), (7, 2), (10, 13), (15, 1), (14, 1), (11,
        1), (10, 1), (8, 1), (0, 112), (15, 2)]),
    "z137": (1, [
        (5, 3), (9, 13), (7, 11), (12, 5), (5, 8), (0, 137), (6, 8), (7, 13), (10, 7), (5, 9), (15, 1), (13,
        1), (11, 1), (10, 1), (8, 1), (7, 1), (6, 1), (0, 33), (15, 2)]),
    "z139": (1, [
        (6, 10), (13, 13), (6, 9), (7, 11), (5, 13), (12, 13), (0, 139), (12, 6), (7, 8), (8, 3), (6, 7),
        (15, 1), (11, 1), (10, 1), (8, 1), (6, 1), (0, 17), (15, 2)]),
    "z141": (0, [
        (8, 12), (11, 13), (5, 9), (7, 13), (8, 10), (14, 8), (5, 13), (6, 7), (13, 13), (12, 2), (0, 141),
        (10, 3), (15, 1), (12, 1), (11, 1), (10, 1), (9, 1), (0, 5), (15, 2)]),
    "z149": (0, [
        (11, 2), (0, 149), (11, 13), (5, 10), (11, 13), (6, 9), (10, 13), (5, 7), (7, 8), (10, 6), (5, 4),
        (6, 5), (15, 1), (13, 1), (12, 1), (11, 1), (9, 1), (8, 1), (7, 1), (6, 1), (0, 7), (15, 2)]),
}
# Three more from counts per length instead of a table: name: (index of the zero run, its
# length, {length: literals}, seed); the lengths 9..15 are there once each (127 bytes), the
# other literals' lengths are shuffled.  NO_RUNS has no zero at all and no equal neighbours
# among its first 249 lengths: 259 lengths in runs of at most 2, so the header has one item per
# length, more than 256, and the emission loop of huff_emit makes five rounds of 64.
RLE_COUNTS = {
    "z138": (0, 138, {6: 30, 7: 54, 8: 27}, 1),
    "z140": (100, 140, {6: 40, 7: 26, 8: 43}, 2),
    "z148": (60, 148, {5: 4, 6: 30, 7: 36, 8: 31}, 3),
    "no_runs": (0, 0, {7: 56, 8: 93, 9: 100}, 4),
}
NO_RUNS = "no_runs"


def _count_lengths(name):
    at, run, counts, seed = RLE_COUNTS[name]
    rng = np.random.default_rng(seed)
    if run:
        body = rng.permutation([l for l, c in counts.items() for _ in range(c)]).tolist()
    else:   # the most frequent length left that differs from the one before
        left, body = dict(counts), []
        while any(left.values()):
            l = max((l for l in left if left[l] and (not body or l != body[-1])), key=lambda l: (left[l], l))
            left[l] -= 1
            body.append(l)
    body += [10, 9, 11, 12, 13, 14, 15] if body[-1] == 9 else [9, 10, 11, 12, 13, 14, 15]
    lens = body[:at] + [0] * run + body[at:]
    assert len(lens) == 256 and (not run or (at == 0 or lens[at - 1]) and lens[at + run])
    return lens


# The one table of (block, classes it owns): ("z" | "n", R) a zero / repeated-length run of R,
# ("zx" | "nx", k) such a run through indices k - 1 and k (a 64-lane register boundary; 256: into
# the end-of-block length), "hlit" a repeat that starts in the lit/len lengths and ends behind
# HLIT, "items" more than 256 header items.  Together they are RLE_REQUIRED: zero runs on both
# sides of 3 / 11 / 138 and of 138 + 3 / 138 + 11 (no zero run passes 255: index 256 always has
# a code), every (R - 1) mod 6 of a repeated length on both sides of 3, and every boundary.
RLE_CLASSES = {
    "small": {("z", r) for r in (1, 2, 3, 10, 11, 12)} | {("n", r) for r in range(1, 12)} | {("n", 13), ("nx", 128)},
    "z137": {("z", 137), ("zx", 64), ("nx", 192), ("nx", 256)},
    "z138": {("z", 138), ("zx", 128)},
    "z139": {("z", 139), ("nx", 64)},
    "z140": {("z", 140), ("zx", 192)},
    "z141": {("z", 141)},
    "z148": {("z", 148)},
    "z149": {("z", 149)},
    "no_runs": {"items"},
    "cross_hlit": {"hlit"},
}
RLE_REQUIRED = ({("z", r) for r in (1, 2, 3, 10, 11, 12, 137, 138, 139, 140, 141, 148, 149)}
                | {("n", r) for r in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13)}
                | {("zx", k) for k in (64, 128, 192)} | {("nx", k) for k in (64, 128, 192, 256)} | {"hlit", "items"})


def rle_lengths(name):
    """The block's 257 lit/len lengths: from its table, or from its counts."""
    if name in RLE_COUNTS:
        return _count_lengths(name) + [15]
    return [l for l, r in RLE_BLOCKS[name][1] for _ in range(r)] + [15]


RLE_NAMES = list(RLE_BLOCKS) + list(RLE_COUNTS)


@functools.lru_cache(maxsize=None)
def rle_blocks():
    out = {}
    for name in RLE_NAMES:
        lens = rle_lengths(name)[:256]
        w = [1 << (15 - l) if l else 0 for l in lens]
        assert len(lens) == 256 and sum(w) == B - 1
        seed = RLE_COUNTS[name][3] if name in RLE_COUNTS else RLE_BLOCKS[name][0]
        pool = np.random.default_rng(seed).permutation(np.repeat(np.arange(256, dtype=np.uint8), w))
        out[name] = _repeat_free(pool.tolist())
    return out


def all_code_inputs():
    """Every block that is about codes: {name: block}."""
    out = {}
    out.update(overflow_ll())
    out.update(overflow_d())
    out.update(overflow_cl())
    out["cross_hlit"] = cross_hlit()
    out.update(rle_blocks())
    return out


# the parses: exhaustive for all; the bounded lazy parse too where the block is built for any parse
PARSES = {name: [(0, False)] + ([(8, True)] if name in ("fib89", "fib144", "dfib17", "dfib18") else [])
          for name in ["fib89", "fib144", "fib233", SHUFFLE, "dfib17", "dfib18", "fib89_shuffle102", "fib89_shuffle130",
                       "fib144_shuffle120", "cross_hlit"] + RLE_NAMES}
