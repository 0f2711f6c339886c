"""Inputs for the segment walk of K1's greedy path (csrc/dmx_walk.h; W1, the Jacobi rounds, W2,
W3 and the one-lane walk of match_block in csrc/dmx_kernels.hip): a background of seeded random
bytes with planted copies at chosen offsets of the 32-position segments, and the list of what
was planted so a test can find each copy in a token stream.

A plant is a position whose token is known by construction.  Every copy is led in by three bytes
that occur nowhere else, so no chance match of the background covers its first position, and is
ended by a byte that differs from the source's (or by the block end).  `lazy_token` /
`greedy_token` say what the position holds in either parse: (length, distance) or None for a
literal.

tests/test_walk_inputs.py checks on the CPU that the oracle's token streams hold every plant;
tests/test_gpu_walk_paths.py holds the GPU to the oracle on the same bytes."""
from collections import namedtuple

import numpy as np

B = 32768
SEG = 32
NSYM = 128          # background alphabet: bytes 0x00 .. 0x7F; the leads use 0x80 and above
MAXLEN = 258
LAST_BN = (1, 2, 3, 31, 32, 33, 63, 64, 65, 32735, 32767)
PERIOD = 37

# block, i: the position; greedy / lazy: (length, distance) of its token, None = a literal;
# kind: the shape it is for
Plant = namedtuple("Plant", "block i greedy lazy kind")


class _Block:
    """One block of n bytes, filled front to back: place() pads with background up to the
    position a record needs."""

    def __init__(self, rng, index, n, nlead):
        self.rng, self.index, self.n = rng, index, n
        self.cur = bytearray()
        self.plants = []
        self.nlead = nlead

    def bg(self, n):
        return bytes(self.rng.integers(0, NSYM, n, dtype=np.uint8).tolist())

    def other(self, *cs):
        d = int(self.rng.integers(0, NSYM))
        while d in cs:
            d = (d + 1) % NSYM
        return d

    def lead(self):
        c = self.nlead
        self.nlead += 1
        return bytes([0x80 + c // 10000, 0x80 + (c // 100) % 100, 0x80 + c % 100])

    def pad_to(self, p):
        assert len(self.cur) <= p <= self.n, (len(self.cur), p, self.n)
        self.cur += self.bg(p - len(self.cur))

    def source(self, body, after):
        """lead, body, one byte that is none of `after`; returns the body's position."""
        self.cur += self.lead()
        q = len(self.cur)
        self.cur += bytes(body) + bytes([self.other(*after)])
        self.cur += self.bg(2)
        return q

    def copy(self, p, length, kind):
        """A copy of `length` bytes at position p exactly (ended by a differing byte, or by the
        block end when p + length == n), its source placed just before it."""
        body = self.bg(length + 1)
        need = 3 + length + 1 + 2 + 3   # source record, lead
        self.pad_to(max(len(self.cur), p - need - int(self.rng.integers(0, 5))))
        q = self.source(body[:length], (body[length],))
        self.pad_to(p - 3)
        self.cur += self.lead()
        assert len(self.cur) == p
        self.cur += body[:length]
        if p + length < self.n:
            self.cur += bytes([self.other(self.cur[q + length], body[length])])
        tok = (min(length, MAXLEN), p - q)
        self.plants.append(Plant(self.index, p, tok, tok, kind))

    def chain(self, p, length, n, kind):
        """Positions p, p + 1, .., p + n - 1 hold copies of length, length + 1, .. (each from a
        source of its own): the lazy rule makes all but the last literals, the greedy parse
        takes the first."""
        text = self.bg(length + 2 * n - 2)
        tail = self.other(text[-1])
        need = sum(3 + length + 2 * j + 1 + 2 for j in range(n)) + 3
        self.pad_to(max(len(self.cur), p - need - int(self.rng.integers(0, 5))))
        qs = []
        for j in range(n):
            end = 2 * j + length
            nxt = text[end] if end < len(text) else tail
            qs.append(self.source(text[j:end], (nxt,)))
        self.pad_to(p - 3)
        self.cur += self.lead()
        assert len(self.cur) == p
        self.cur += text + bytes([tail])
        for j in range(n):
            g = (length, p - qs[0]) if j == 0 else None   # greedy: the first copy covers the others' starts
            lz = (length + 2 * (n - 1) - (n - 1), p + n - 1 - qs[n - 1]) if j == n - 1 else None
            self.plants.append(Plant(self.index, p + j, g, lz, kind))

    def close(self):
        self.pad_to(self.n)
        return bytes(self.cur)


def _main_input(rng):
    """Three blocks, the last one short: shapes 1-6 and 8."""
    blocks, plants, nlead = [], [], 0
    for b, n in enumerate((B, B, 20000 + 7)):
        k = _Block(rng, b, n, nlead)
        s = 8 + 3 * b   # the first segments stay literals (shape 5)
        # 1: literals up to a segment end, a match at offset 0 of the next
        k.copy(SEG * s, 5 + b, "lit-run-then-match-at-0")
        s += 3
        # 2: a match that starts at offset 31
        for ln in (3, 4, 40 + b):
            k.copy(SEG * s + 31, ln, "match-at-31")
            s += 4
        # 3: a match that ends exactly on a segment boundary
        for off, ln in ((10, 22), (29, 3), (29, 35), (0, 32), (0, 64)):
            k.copy(SEG * s + off, ln, "match-ends-on-boundary")
            s += 5
        # 4: a match of 258 over eight segments (and longer copies, cut at 258)
        s += 10
        for off, ln in ((5, 258), (31, 258), (0, 300)):
            k.copy(SEG * s + off, ln, "match-258")
            s += 20
        # 8: lazy pairs and chains of three across the boundary
        for n_chain in (2, 3):
            for off in (29, 30, 31):
                for ln in (3, 4, 9):
                    k.chain(SEG * s + off, ln + b, n_chain, f"lazy-chain-{n_chain}")
                    s += 5
        # a match over a boundary that ends inside the next segment
        k.copy(SEG * s + 20, 15, "match-over-boundary")
        s += 3
        # 6: a match that ends exactly at bn
        k.pad_to(n - 600)
        k.copy(n - 40 - b, 40 + b, "match-ends-at-bn")
        blocks.append(k.close())
        plants += k.plants
        nlead = k.nlead
    return b"".join(blocks), plants


def _last_block_input(rng, bn):
    """A full background block and a last block of bn bytes.  Short ones repeat five bytes, so
    that a match runs from position 5 to bn exactly; long ones hold a copy ending at bn."""
    first = _Block(rng, 0, B, 0)
    first.copy(SEG * 9 + 31, 7, "match-at-31")
    blocks, plants = [first.close()], list(first.plants)
    if bn <= 65:
        unit = bytes([0x90, 0x91, 0x92, 0x93, 0x94])
        blk = (unit * 14)[:bn]
        if bn >= 8:
            tok = (bn - 5, 5)
            plants.append(Plant(1, 5, tok, tok, "match-ends-at-bn"))
        blocks.append(blk)
    else:
        k = _Block(rng, 1, bn, first.nlead)
        k.copy(SEG * 11, 6, "lit-run-then-match-at-0")
        k.pad_to(bn - 700)
        k.copy(bn - 258, 258, "match-ends-at-bn")
        blocks.append(k.close())
        plants += k.plants
    return b"".join(blocks), plants


def periodic_block(head=0, seed=0x37):
    """Shape 9 (head = 0): one block of period-37 data, so every position from 37 on holds a
    258-byte match and the block has fewer than 1024 tokens.  Shape 10 (head = 2048): the same
    behind `head` random bytes, so it has more than 1024 tokens."""
    rng = np.random.default_rng(seed)
    unit = bytes(rng.permutation(NSYM)[:PERIOD].astype(np.uint8).tolist())
    h = bytes(rng.integers(0x80, 0x100, head, dtype=np.uint8).tolist())
    return h + (unit * (B // PERIOD + 1))[:B - head]


def build(seed=0x3A1C):
    """[(name, data, plants)]: every input of one to three blocks."""
    rng = np.random.default_rng(seed)
    out = [("main",) + _main_input(rng)]
    for bn in LAST_BN:
        out.append((f"last-{bn}",) + _last_block_input(rng, bn))
    return out


def tokens_at(tok):
    """{position: (length, distance) or None} of a token stream (uint32: dist << 9 | len)."""
    at, p = {}, 0
    for t in np.asarray(tok, dtype=np.uint32).tolist():
        d = t >> 9
        at[p] = (t & 0x1FF, d) if d else None
        p += (t & 0x1FF) if d else 1
    return at


def find_plants(tokens_per_block, plants, lazy):
    """The plants missing from per-block token streams: a plant is found when its position
    starts a token of the planted kind (a literal, or a match of its length and distance).  A
    plant the parse does not start a token at (greedy: inside the first copy of a chain) is
    found when no token starts there."""
    missing = []
    for b, tok in enumerate(tokens_per_block):
        at = tokens_at(tok)
        for pl in plants:
            if pl.block != b:
                continue
            want = pl.lazy if lazy else pl.greedy
            if not lazy and want is None and pl.kind.startswith("lazy-chain"):
                if pl.i in at:
                    missing.append((pl, at[pl.i]))
            elif pl.i not in at or at[pl.i] != want:
                missing.append((pl, at.get(pl.i, "no token")))
    return missing
