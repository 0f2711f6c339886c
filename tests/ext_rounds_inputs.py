"""Inputs for the match extension's rounds (ext_len2 in csrc/dmx_kernels.hip: 24 bytes in the
first LDS round trip after the 8 register bytes, then 32 per round trip): a seeded 40-symbol
background with planted copies, and the list of what was planted so a test can find each copy
in a token stream.

A plant is a position i whose longest match is known by construction: `length` bytes at
distance `dist`, ended by a differing byte or by the block end.  Each copy is led in by three
bytes that occur nowhere else, so no chance match of the background covers position i and the
copy starts a token in the greedy and in the lazy parse alike.

tests/test_ext_rounds_inputs.py checks on the CPU that the oracle's token streams hold every
plant; tests/test_gpu_ext_rounds.py holds the GPU to the oracle on the same bytes."""
from collections import namedtuple

import numpy as np

B = 32768
NSYM = 40           # background alphabet: bytes 0x30 .. 0x57
SYM0 = 0x30
LENGTHS = (8, 9, 10, 11, 12, 31, 32, 33, 34, 35, 63, 64, 65, 95, 96, 97, 255, 256, 257, 258, 259, 300)
END_GAPS = (9, 10, 31, 32, 33, 257, 258, 259)   # bn - i of the copies that run into a block's end
SHORT_LAST = 20011                               # bytes of the short last block
TRIPLE_L = (20, 31, 32, 40)                      # L of the three-source plants: both sides of 8 + 24
MAXLEN = 258

# block: index of the 32 KiB block; i: offset in the block; kind: what the plant is for;
# hist: the source lies in the previous block (found only with DMX_F_DICT)
Plant = namedtuple("Plant", "block i length dist kind hist")


def bucket(b0, b1, b2):
    """The GPU's 13-bit multiplicative hash of a trigram."""
    return (((b0 | b1 << 8 | b2 << 16) * 0x9E3779B1) & 0xFFFFFFFF) >> 19


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.blocks = []      # finished blocks (bytearrays)
        self.cur = bytearray()
        self.plants = []
        self.nlead = 0

    def bg(self, n):
        return bytes((self.rng.integers(0, NSYM, n, dtype=np.uint8) + SYM0).tolist())

    def other(self, c):
        """A background symbol that is not c."""
        d = SYM0 + int(self.rng.integers(0, NSYM))
        return d if d != c else SYM0 + (d - SYM0 + 1) % NSYM

    def lead(self):
        """Three bytes outside the background alphabet; no two leads share a byte pair."""
        c = self.nlead
        self.nlead += 1
        return bytes([0x80 + c // 10000, 0x80 + (c // 100) % 100, 0x80 + c % 100])

    def pad_to(self, mod4):
        while len(self.cur) % 4 != mod4:
            self.cur += self.bg(1)

    def room(self):
        return B - len(self.cur)

    def close_block(self, n=B):
        if len(self.cur) < n:
            self.cur += self.bg(n - len(self.cur))
        assert len(self.cur) == n
        self.blocks.append(self.cur)
        self.cur = bytearray()

    def copy_record(self, length, qa, ia, kind, reserve):
        """source (qa = q mod 4), a differing byte, background, lead, the copy (ia = i mod 4),
        a differing byte.  Goes to the next block if this one has no room left above `reserve`."""
        need = 2 * (length + 1) + 40
        if self.room() < need + reserve:
            return False
        body = self.bg(length + 1)
        self.pad_to(qa)
        q = len(self.cur)
        self.cur += body
        self.cur += self.bg(int(self.rng.integers(3, 12)))
        self.pad_to((ia - 3) % 4)
        self.cur += self.lead()
        i = len(self.cur)
        assert i % 4 == ia and q % 4 == qa
        self.cur += body[:length] + bytes([self.other(body[length])])
        self.plants.append(Plant(len(self.blocks), i, min(length, MAXLEN), i - q, kind, False))
        self.cur += self.bg(int(self.rng.integers(2, 9)))
        return True

    def triple_record(self, lens, kind, first=None):
        """Three sources (far, middle, nearest) of one position; lens = (nearest, middle, far).
        first: the three bytes every copy starts with (a chosen bucket), else background."""
        lmax = max(lens)
        body = bytearray(self.bg(lmax + 1))
        if first is not None:
            body[:3] = first
        for ln in (lens[2], lens[1], lens[0]):
            self.cur += bytes(body[:ln]) + bytes([self.other(body[ln])]) + self.lead()
        i = len(self.cur)
        self.cur += body   # (differs from every source at that source's length)
        # the longest source wins, the nearest of those that tie (strict > along the chain)
        best = max(lens)
        j = [lens[0], lens[1], lens[2]].index(best)   # 0 = nearest
        # distances: each source record is ln + 1 + 3 bytes long
        ends = []
        p = i
        for ln in (lens[0], lens[1], lens[2]):
            p -= ln + 1 + 3
            ends.append(p)
        self.plants.append(Plant(len(self.blocks), i, best, i - ends[j], kind, False))
        self.cur += self.bg(int(self.rng.integers(2, 9)))

    def end_record(self, gap, n=B):
        """A copy whose last `gap` bytes end the block (of n bytes); the source goes on matching
        into bytes the block no longer has."""
        src_len = gap + 8
        i = n - gap
        start = i - 3 - 16 - src_len
        assert len(self.cur) <= start, (len(self.cur), start)
        self.cur += self.bg(start - len(self.cur))
        q = len(self.cur)
        body = self.bg(src_len)
        self.cur += body + self.bg(16) + self.lead()
        assert len(self.cur) == i
        self.cur += body[:gap]
        self.plants.append(Plant(len(self.blocks), i, min(gap, MAXLEN), i - q, "end", False))
        self.close_block(n)


def low_bucket_trigram():
    """Three bytes outside the background alphabet (and the leads' range) that hash to bucket 0:
    entries of that bucket are the first of S."""
    for a in range(0xE8, 0x100):
        for b in range(0xE8, 0x100):
            for c in range(0xE8, 0x100):
                if bucket(a, b, c) == 0:
                    return bytes([a, b, c])
    raise AssertionError("no trigram of bucket 0")


def build(seed=0x0E17):
    """(data, plants): eight blocks, the last one short."""
    bd = _Builder(seed)
    recs = [(ln, qa, ia) for ln in LENGTHS for qa in range(4) for ia in range(4)]
    order = bd.rng.permutation(len(recs))
    todo = [recs[k] for k in order]
    t0 = low_bucket_trigram()
    triples = [(kind, L) for L in TRIPLE_L for kind in ("LLL", "LMM", "LLF", "NLL")]

    def lens_of(kind, L):
        return {"LLL": (L, L, L), "LMM": (L, L + 1, L + 1), "LLF": (L, L, L + 40), "NLL": (L + 1, L, L)}[kind]

    nblk = len(END_GAPS)
    for b in range(nblk):
        n = B if b < nblk - 1 else SHORT_LAST
        gap = END_GAPS[b]
        reserve = (B - n) + 2 * gap + 8 + 3 + 16 + 8
        if b in (1, 3):
            # the block's first entries of S: sources and copy in bucket 0, from offset 0 on
            L = TRIPLE_L[b // 2]
            bd.triple_record(lens_of("LMM", L), "first", first=t0)
        if b >= 1:
            # sources at the end of the previous block for copies at the start of this one
            for ln, back in ((8 + 4 * b + b % 4, 40), (33 + b, 300), (258 + b % 2, 700)):
                prev = bytes(bd.blocks[b - 1])
                while prev.count(prev[B - back - ln - 8:B - back - 8]) != 1:   # (not inside a planted copy)
                    back += 61
                src = prev[B - back - ln - 8:B - back - 8 + 1]
                bd.cur += bd.bg(int(bd.rng.integers(1, 5))) + bd.lead()
                i = len(bd.cur)
                bd.cur += src[:ln] + bytes([bd.other(src[ln])])
                bd.plants.append(Plant(b, i, min(ln, MAXLEN), i + B - (B - back - ln - 8), "hist", True))
                bd.cur += bd.bg(5)
        while triples and b % 2 == 0 and bd.room() > reserve + 400:
            kind, L = triples.pop()
            bd.triple_record(lens_of(kind, L), kind)
            if len(triples) % 4 == 0:
                break
        while todo:
            ln, qa, ia = todo[-1]
            if not bd.copy_record(ln, qa, ia, "len", reserve):
                break
            todo.pop()
        bd.end_record(gap, n)
    assert not todo and not triples, (len(todo), len(triples))
    data = b"".join(bytes(x) for x in bd.blocks)
    assert len(data) == (nblk - 1) * B + SHORT_LAST
    return data, bd.plants


def find_plants(tokens_per_block, plants, with_hist):
    """The plants missing from per-block token streams (uint32: dist << 9 | len, dist 0 = a
    literal): a plant is found when a match token starts at its position with its length and
    distance.  Plants whose source is in the previous block count only with_hist."""
    missing = []
    for b, tok in enumerate(tokens_per_block):
        at = {}
        p = 0
        for t in np.asarray(tok, dtype=np.uint32).tolist():
            d = t >> 9
            if d:
                at[p] = (t & 0x1FF, d)
                p += t & 0x1FF
            else:
                p += 1
        for pl in plants:
            if pl.block == b and (with_hist or not pl.hist) and at.get(pl.i) != (pl.length, pl.dist):
                missing.append((pl, at.get(pl.i)))
    return missing
