"""A bit-level DEFLATE writer and the hand-built corpus of the inflate conformance tests.

Encoders leave large parts of RFC 1951 unused (distances above 32506, repeat runs across the
HLIT/HDIST boundary, incomplete codes, the reserved fixed-code symbols ...), so the decoders
(csrc/dmx_inflate.c, csrc/dmx_inflate_dev.hip) are pinned on streams spelled bit by bit here:

    Deflate                 LSB-first bit writer; Huffman codes go out MSB-first
      .stored(data, final)
      .fixed_block(items, final)
      .dynamic_block(ll_lens, d_lens, items, cl_lens=CL_PLAIN, cl_syms=None, final=True)
    canonical(lens)         canonical code assignment from a list of lengths
    zlib_wrap(raw, data)    78 9C + raw + Adler-32(data)
    parse_dynamic_header    the RFC 1951 3.2.7 header of a stream's first block, for self-checks
    CASES                   [(name, raw_deflate, kind)], kind "valid" / "invalid"; built at import
    zstream(name)           the case as a zlib stream (junk / a wrong Adler-32 where the case is that)

`items` of a block: ("L", sym) a literal/length symbol, ("D", sym) a distance symbol,
("X", value, nbits) raw extra bits, ("C", code, nbits) a raw code written MSB-first (a bit
pattern no symbol owns).  match(length, dist) spells the four items of a match.

Plain Python, imported like golden_inputs.py; deterministic (numpy's seeded generator).
"""
import heapq
import struct
import zlib

import numpy as np

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# the two code-length codes of the corpus, both Kraft-complete
CL_RLE = {16: 3, 17: 3, 18: 3, **{k: 4 for k in range(10)}}     # 3/8 + 10/16
CL_PLAIN = {k: 4 for k in range(16)}                            # 16/16

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
         4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]

FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32   # 30 and 31 have codes and no meaning


def canonical(lens):
    """{symbol: (code, length)} by RFC 1951 3.2.2.  An over-subscribed list still gets codes
    (they overflow their length and are masked): such a block is rejected before any is read."""
    lens = list(lens)
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n] & ((1 << n) - 1), n)
            nxt[n] += 1
    return out


def kraft(lens):
    """Sum of 2^-len over the coded symbols, in units of 2^-15 (complete: 32768)."""
    return sum(1 << (15 - n) for n in lens if n)


def complete_lens(syms, n):
    """A Kraft-complete list of n lengths with codes for exactly `syms` (two or more)."""
    syms = sorted(set(syms))
    k = len(syms)
    assert k >= 2
    top = (k - 1).bit_length()
    short = (1 << top) - k
    lens = [0] * n
    for j, s in enumerate(syms):
        lens[s] = top - 1 if j < short else top
    assert kraft(lens) == 32768
    return lens


def huffman_lens(freq, n):
    """Huffman code lengths of the symbols with a count (two or more of them)."""
    heap = [(f, s, (s,)) for s, f in sorted(freq.items()) if f]
    assert len(heap) >= 2
    heapq.heapify(heap)
    lens = [0] * n
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    assert max(lens) <= 15 and kraft(lens) == 32768
    return lens


def len_sym(length):
    if length == 258:
        return 285, 0, 0
    k = max(j for j in range(28) if LBASE[j] <= length)
    return 257 + k, length - LBASE[k], LEXT[k]


def dist_sym(dist):
    k = max(j for j in range(30) if DBASE[j] <= dist)
    return k, dist - DBASE[k], DEXT[k]


def match(length, dist, lsym=None):
    """The items of a match; lsym = (symbol, extra value) picks another spelling of the length."""
    ls, lx, ln = len_sym(length)
    if lsym is not None:
        ls, lx = lsym
        ln = LEXT[ls - 257]
        assert LBASE[ls - 257] + lx == length
    ds, dx, dn = dist_sym(dist)
    return [("L", ls), ("X", lx, ln), ("D", ds), ("X", dx, dn)]


def lits(data):
    return [("L", b) for b in data]


def cl_zeros(n):
    """Code-length symbols for n zeros: 18s, a 17, plain zeros."""
    out = []
    while n >= 11:
        k = min(n, 138)
        out.append((18, k - 11))
        n -= k
    if n >= 3:
        out.append((17, n - 3))
        n = 0
    return out + [0] * n


def cl_expand(cl_syms):
    """The lengths a code-length symbol sequence spells."""
    lens = []
    for s in cl_syms:
        if isinstance(s, int):
            lens.append(s)
        elif s[0] == 16:
            lens += [lens[-1]] * (3 + s[1])
        elif s[0] == 17:
            lens += [0] * (3 + s[1])
        else:
            lens += [0] * (11 + s[1])
    return lens


def cl_rle(lens):
    """A plain run-length spelling of a list of lengths (16 / 17 / 18 where they fit)."""
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        run = j - i
        if lens[i] == 0:
            out += cl_zeros(run)
        else:
            out.append(lens[i])
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [lens[i]] * run
        i = j
    return out


class Deflate:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def bits(self, v, n):
        """n bits of v, least significant first."""
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, c, n):
        """A Huffman code of n bits, most significant first."""
        r = 0
        for k in range(n):
            r |= ((c >> k) & 1) << (n - 1 - k)
        return self.bits(r, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")

    # ---- blocks
    def stored(self, data, final, nlen=None):
        self.bits(1 if final else 0, 1).bits(0, 2).align()
        self.bits(len(data), 16).bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.buf += data
        return self

    def _items(self, items, ll, dd):
        for it in items:
            if it[0] == "L":
                self.code(*ll[it[1]])
            elif it[0] == "D":
                self.code(*dd[it[1]])
            elif it[0] == "X":
                self.bits(it[1], it[2])
            else:
                self.code(it[1], it[2])
        return self

    def fixed_block(self, items, final):
        self.bits(1 if final else 0, 1).bits(1, 2)
        return self._items(items, canonical(FIXED_LL), canonical(FIXED_D))

    def dynamic_block(self, ll_lens, d_lens, items, cl_lens=None, cl_syms=None, final=True):
        """HLIT = len(ll_lens) - 257 and HDIST = len(d_lens) - 1, written as they are (5 bits:
        up to 288 / 32).  cl_syms spells the code-length sequence itself -- a length, or
        (16 | 17 | 18, extra-bits value); by default every length is written plainly."""
        cl_lens = dict(CL_PLAIN if cl_lens is None else cl_lens)
        if cl_syms is None:
            cl_syms = list(ll_lens) + list(d_lens)
        used = [k for k in range(19) if cl_lens.get(CL_ORDER[k], 0)]
        hclen = max(4, used[-1] + 1 if used else 4)
        self.bits(1 if final else 0, 1).bits(2, 2)
        self.bits(len(ll_lens) - 257, 5).bits(len(d_lens) - 1, 5).bits(hclen - 4, 4)
        for k in range(hclen):
            self.bits(cl_lens.get(CL_ORDER[k], 0), 3)
        cc = canonical([cl_lens.get(s, 0) for s in range(19)])
        for s in cl_syms:
            if isinstance(s, int):
                self.code(*cc[s])
            else:
                self.code(*cc[s[0]])
                self.bits(s[1], {16: 2, 17: 3, 18: 7}[s[0]])
        return self._items(items, canonical(ll_lens), canonical(d_lens))


def zlib_wrap(raw, data=b""):
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data))


# ------------------------------------------------------------------------------------------
# Header parser (self-checks; test_gpu_inflate's long-code check)
# ------------------------------------------------------------------------------------------
def parse_dynamic_header(z, raw_offset=2):
    """The header of the first DEFLATE block at byte raw_offset of z.  None if it is not a
    dynamic block; otherwise a dict: hlit, hdist, hclen, cl_lens (19), ops [(code-length symbol,
    first index, count)], lens (as far as they were spelled), ll / dd (the two lists, when all
    lengths are there), bad (why the code-length sequence stopped, or None)."""
    pos = raw_offset * 8

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            byte = z[(pos + i) >> 3] if (pos + i) >> 3 < len(z) else 0
            v |= ((byte >> ((pos + i) & 7)) & 1) << i
        pos += n
        return v

    bits(1)
    if bits(2) != 2:
        return None
    h = {"hlit": bits(5) + 257, "hdist": bits(5) + 1, "hclen": bits(4) + 4, "ops": [], "lens": [], "bad": None,
         "ll": None, "dd": None}
    cl = [0] * 19
    for k in range(h["hclen"]):
        cl[CL_ORDER[k]] = bits(3)
    h["cl_lens"] = cl
    total = h["hlit"] + h["hdist"]
    if h["hlit"] > 286 or h["hdist"] > 30:
        h["bad"] = "too many symbols"
        return h
    if kraft(cl) != 32768:
        h["bad"] = "code-length code not complete"
        return h
    codes = {v: s for s, v in canonical(cl).items()}
    lens = h["lens"]
    while len(lens) < total:
        c, n = 0, 0
        while (c, n) not in codes:
            c = (c << 1) | bits(1)
            n += 1
            assert n <= 7
        s = codes[(c, n)]
        if s < 16:
            h["ops"].append((s, len(lens), 1))
            lens.append(s)
            continue
        if s == 16 and not lens:
            h["bad"] = "16 first"
            return h
        rep = 3 + bits(2) if s == 16 else 3 + bits(3) if s == 17 else 11 + bits(7)
        h["ops"].append((s, len(lens), rep))
        if len(lens) + rep > total:
            h["bad"] = "repeat past the end"
            return h
        lens += [lens[-1] if s == 16 else 0] * rep
    h["ll"], h["dd"] = lens[:h["hlit"]], lens[h["hlit"]:]
    h["end_bit"] = pos
    return h


def max_code_lengths(z, raw_offset=2):
    """(longest literal/length code, longest distance code) of the first block of a zlib
    stream, or None if that block is not dynamic."""
    h = parse_dynamic_header(z, raw_offset)
    return None if h is None else (max(h["ll"]), max(h["dd"]))


# ------------------------------------------------------------------------------------------
# A small encoder on top of the writer: the streams of the truncation and bit-flip sweeps
# ------------------------------------------------------------------------------------------
def _tokens(data, min_len=3):
    """Greedy longest-match parse (quadratic: for a few hundred bytes)."""
    out, i = [], 0
    while i < len(data):
        best, bd = 0, 0
        for j in range(max(0, i - 32768), i):
            k = 0
            while k < 258 and i + k < len(data) and data[j + k] == data[i + k]:
                k += 1
            if k >= best and k >= min_len:
                best, bd = k, i - j
        if best:
            out.append((best, bd))
            i += best
        else:
            out.append(data[i])
            i += 1
    return out


def encode_dynamic(data):
    """One final dynamic block for data: greedy parse, Huffman lengths, the run-length code-length code."""
    items, fl, fd = [], {256: 1}, {}
    for t in _tokens(data):
        if isinstance(t, int):
            items.append(("L", t))
            fl[t] = fl.get(t, 0) + 1
        else:
            m = match(*t)
            items += m
            fl[m[0][1]] = fl.get(m[0][1], 0) + 1
            fd[m[2][1]] = fd.get(m[2][1], 0) + 1
    items.append(("L", 256))
    ll = huffman_lens(fl, max(fl) + 1)
    ll += [0] * (257 - len(ll))
    if len(fd) >= 2:
        dd = huffman_lens(fd, max(fd) + 1)
    else:
        dd = [0] * (max(fd) + 1 if fd else 1)
        if fd:
            dd[-1] = 1
    assert max(ll + dd) <= 9
    return Deflate().dynamic_block(ll, dd, items, cl_lens=CL_RLE, cl_syms=cl_rle(ll + dd)).getvalue()


def _sweep_text(n, seed):
    rng = np.random.default_rng(seed)
    words = [b"block", b"code", b"length", b"distance", b"window", b"literal", b"the", b"of", b"a", b"stream"]
    out = b""
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + b" "
    return out[:n]


def sweep_streams():
    """{name: (zlib stream, data)}: three complete streams under 120 bytes for the truncation
    sweep (fixed, dynamic, stored) and one dynamic stream of about 300 bytes for the bit flips."""
    t = _sweep_text(150, 1)
    items = []
    for tok in _tokens(t):
        items += [("L", tok)] if isinstance(tok, int) else match(*tok)
    fixed = Deflate().fixed_block(items + [("L", 256)], True).getvalue()
    s = _sweep_text(90, 2)
    big = _sweep_text(1200, 3)
    out = {
        "fixed": (zlib_wrap(fixed, t), t),
        "dynamic": (zlib_wrap(encode_dynamic(t), t), t),
        "stored": (zlib_wrap(Deflate().stored(s[:40], False).stored(s[40:], True).getvalue(), s), s),
        "flip": (zlib_wrap(encode_dynamic(big), big), big),
    }
    for k in ("fixed", "dynamic", "stored"):
        assert len(out[k][0]) < 120, (k, len(out[k][0]))
    assert 250 <= len(out["flip"][0]) <= 350, len(out["flip"][0])
    return out


# ------------------------------------------------------------------------------------------
# The corpus
# ------------------------------------------------------------------------------------------
CASES = []            # (name, raw DEFLATE, "valid" | "invalid")
WRAPPED = {}          # name -> the zlib stream, where it is not zlib_wrap(raw, expected)
HEADER_CHECKS = {}    # name -> predicate on parse_dynamic_header(zstream): the property the case claims
ZLIB_SAYS = {}        # name -> zlib's error text (invalid cases): the reason, not only the verdict
EARLY = set()         # invalid cases whose error precedes any output byte
EXPECT = {}           # name -> the bytes the case spells (where they are cheap to state)
BIT_OFFSET = {}       # name -> (bit position in the raw stream of a block header, claimed position mod 8)
_RAW = {}


def _add(name, raw, kind, says=None, early=False, check=None, expect=None):
    if isinstance(raw, Deflate):
        raw = raw.getvalue()
    assert name not in _RAW
    CASES.append((name, raw, kind))
    _RAW[name] = raw
    if says:
        ZLIB_SAYS[name] = says
    if early:
        assert kind == "invalid"
        EARLY.add(name)
    if check:
        HEADER_CHECKS[name] = check
    if expect is not None:
        EXPECT[name] = expect


def expected(name):
    """zlib's bytes of a valid case (the reference), b"" for an invalid one."""
    kind = next(k for n, _, k in CASES if n == name)
    return zlib.decompress(_RAW[name], -15) if kind == "valid" else b""


def zstream(name):
    return WRAPPED[name] if name in WRAPPED else zlib_wrap(_RAW[name], expected(name))


def _nz(lens):
    return {s: n for s, n in enumerate(lens) if n}


def _ll(syms):
    return complete_lens(syms, 257 if max(syms) <= 256 else max(syms) + 1)


def _build():
    rng = np.random.default_rng(1951)
    A, B, EOB = 97, 98, 256
    ll_ab = _ll([A, B, EOB, 257])                 # four codes of length 2
    assert _nz(ll_ab) == {A: 2, B: 2, EOB: 2, 257: 2}
    ll_am = _ll([A, EOB, 257])                    # a: 1, EOB and 257: 2

    # ---- valid
    _add("hdist1_zero_literals", Deflate().dynamic_block(_ll(list(b"helo") + [EOB]), [0], lits(b"hello") + [("L", EOB)]),
         "valid", expect=b"hello", check=lambda h: h["hdist"] == 1 and h["dd"] == [0])
    _add("eob_only_len1", Deflate().dynamic_block([0] * 256 + [1], [0], [("L", EOB)]), "valid", expect=b"",
         check=lambda h: _nz(h["ll"]) == {EOB: 1} and _nz(h["dd"]) == {})
    _add("single_dist_len1", Deflate().dynamic_block(ll_am, [1], [("L", A)] + match(3, 1) + [("L", EOB)]), "valid",
         expect=b"aaaa", check=lambda h: h["dd"] == [1])
    # a 16 that starts on the last literal/length lengths and ends in the distance lengths
    syms = cl_zeros(97) + [2, 2] + cl_zeros(157) + [2, (16, 2)]
    assert cl_expand(syms) == ll_ab + [2, 2, 2, 2]
    _add("rep16_across_hlit", Deflate().dynamic_block(ll_ab, [2] * 4, lits(b"ab") + match(3, 2) + [("L", EOB)],
                                                      cl_lens=CL_RLE, cl_syms=syms), "valid", expect=b"ababa",
         check=lambda h: any(s == 16 and i < h["hlit"] < i + c for s, i, c in h["ops"]))
    # a 16 straight after a 17: it repeats the 17's zero
    syms = [(17, 0), (16, 0)] + cl_zeros(91) + [2, 2] + cl_zeros(157) + [2, 2, 1, 1]
    assert cl_expand(syms) == ll_ab + [1, 1]
    _add("rep16_after_17", Deflate().dynamic_block(ll_ab, [1, 1], lits(b"ab") + match(3, 2) + [("L", EOB)],
                                                   cl_lens=CL_RLE, cl_syms=syms), "valid", expect=b"ababa",
         check=lambda h: h["ops"][0][0] == 17 and h["ops"][1] == (16, 3, 3) and h["lens"][:6] == [0] * 6)
    ll = [0] * 138 + complete_lens(range(138, 257), 257)[138:]
    syms = [(18, 127)] + ll[138:] + [0]
    _add("rep18_138", Deflate().dynamic_block(ll, [0], lits(bytes(range(138, 256))) + [("L", EOB)], cl_lens=CL_RLE,
                                              cl_syms=syms), "valid", expect=bytes(range(138, 256)),
         check=lambda h: h["ops"][0] == (18, 0, 138))
    # every literal/length and distance symbol has a code
    ll, dd = complete_lens(range(286), 286), complete_lens(range(30), 30)
    items, n = lits(bytes(range(48, 58)) * 30), 300
    for k in range(29):
        length = LBASE[k] + (1 << LEXT[k]) - 1
        d = min(DBASE[min(k, 16)] + (1 << DEXT[min(k, 16)]) - 1, n)
        items += match(length, d, (257 + k, length - LBASE[k]))
        n += length
    _add("hlit286_hdist30_all_assigned", Deflate().dynamic_block(ll, dd, items + [("L", EOB)]), "valid",
         check=lambda h: h["hlit"] == 286 and h["hdist"] == 30 and all(h["ll"]) and all(h["dd"]))
    # codes of every length 1..15 in both tables, the long ones on length and distance symbols
    order = [A, 257, B, EOB, 99, 258, 100, 264, 101, 265, 102, 270, 280, 284, 285, 103]
    ll = [0] * 286
    for k, s in enumerate(order):
        ll[s] = min(k + 1, 15)
    dd = [15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 15]
    assert kraft(ll) == 32768 and kraft(dd) == 32768
    items = lits(b"abcdefg" * 40)   # 280 bytes of history: every distance up to 256 is inside it
    lsyms = [257, 258, 264, 265, 270, 280, 284, 285]
    for ds in range(16):
        for ls in (lsyms[ds % 8], lsyms[(ds + 3) % 8]):
            lx = (ds * 5) % (1 << LEXT[ls - 257])
            dx = (ds * 7) % (1 << DEXT[ds])
            items += [("L", ls), ("X", lx, LEXT[ls - 257]), ("D", ds), ("X", dx, DEXT[ds])]
        items += lits(b"gfedcba")
    _add("code_lengths_1_to_15", Deflate().dynamic_block(ll, dd, items + [("L", EOB)]), "valid",
         check=lambda h: set(h["ll"]) >= set(range(1, 16)) and set(h["dd"]) >= set(range(1, 16)))
    _add("len258_sym285", Deflate().fixed_block(lits(b"x") + match(258, 1) + [("L", EOB)], True), "valid", expect=b"x" * 259)
    _add("len258_sym284_extra31", Deflate().fixed_block(lits(b"x") + match(258, 1, (284, 31)) + [("L", EOB)], True), "valid",
         expect=b"x" * 259)
    _add("dist1_len258_x3", Deflate().fixed_block(lits(b"q") + match(258, 1) * 3 + [("L", EOB)], True), "valid",
         expect=b"q" * 775)
    head = bytes(range(33, 96))
    items, want = lits(head), bytearray(head)
    for d in range(2, 64):
        items += match(258, d)
        for _ in range(258):
            want.append(want[-d])
    _add("dist2_63_len258", Deflate().fixed_block(items + [("L", EOB)], True), "valid", expect=bytes(want))
    # the far end of the window: a stored block of history, then one fixed-block match
    hist = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    for d in (32768, 32767, 32507):
        _add(f"stored32768_dist{d}", Deflate().stored(hist, False).fixed_block(match(258, d) + [("L", EOB)], True), "valid",
             expect=hist + hist[32768 - d:][:258])
    _add("stored32510_dist32507", Deflate().stored(hist[:32510], False).fixed_block(match(258, 32507) + [("L", EOB)], True),
         "valid", expect=hist[:32510] + hist[3:261])
    w = Deflate()
    for _ in range(1000):
        w.stored(b"", False)
    _add("empty_stored_x1000_then_literal", w.fixed_block(lits(b"z") + [("L", EOB)], True), "valid", expect=b"z")
    _add("empty_stored_then_fixed", Deflate().stored(b"", False).fixed_block(lits(b"ok") + [("L", EOB)], True), "valid",
         expect=b"ok")
    big = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    _add("stored65535", Deflate().stored(big, True), "valid", expect=big)
    for k in range(1, 8):
        # the fixed block is 3 + 7 bits and its literals: 8 bits below 144, 9 bits from 144 on
        nine = (k - 2) % 8
        text = b"ab" + bytes([200] * nine)
        w = Deflate().fixed_block(lits(text) + [("L", EOB)], False)
        BIT_OFFSET[f"stored_at_bit{k}_after_fixed"] = (w.bitpos, k)
        _add(f"stored_at_bit{k}_after_fixed", w.stored(b"tail", True), "valid", expect=text + b"tail")
    hello = Deflate().fixed_block(lits(b"hello") + [("L", EOB)], True).getvalue()
    _add("junk_after_trailer", hello, "valid", expect=b"hello")
    WRAPPED["junk_after_trailer"] = zlib_wrap(hello, b"hello") + b"JUNK"

    # ---- invalid
    over = lambda lens: kraft(lens) > 32768
    part = lambda lens: 0 < kraft(lens) < 32768
    ll = [0] * 257
    ll[A] = ll[B] = ll[EOB] = 1
    _add("oversubscribed_ll", Deflate().dynamic_block(ll, [0], lits(b"ab") + [("L", EOB)]), "invalid",
         "invalid literal/lengths set", early=True, check=lambda h: over(h["ll"]))
    _add("oversubscribed_dist", Deflate().dynamic_block(_ll([A, EOB]), [1, 1, 1], lits(b"a") + [("L", EOB)]), "invalid",
         "invalid distances set", early=True, check=lambda h: over(h["dd"]) and kraft(h["ll"]) == 32768)
    _add("oversubscribed_cl", Deflate().dynamic_block(_ll([A, EOB]), [0], [("X", 0, 32)], cl_lens={0: 1, 1: 1, 2: 1},
                                                      cl_syms=[]), "invalid", "invalid code lengths set", early=True,
         check=lambda h: over(h["cl_lens"]))
    _add("incomplete_cl", Deflate().dynamic_block(_ll([A, EOB]), [0], [("X", 0, 32)], cl_lens={0: 2, 1: 2, 2: 2},
                                                  cl_syms=[]), "invalid", "invalid code lengths set", early=True,
         check=lambda h: part(h["cl_lens"]))
    # (zlib reads an empty code-length code as all zeros and then misses the end-of-block code)
    _add("empty_cl", Deflate().dynamic_block(_ll([A, EOB]), [0], [("X", 0, 32)] * 12, cl_lens={}, cl_syms=[]), "invalid",
         early=True, check=lambda h: not any(h["cl_lens"]))
    ll = [0] * 257
    ll[A] = ll[EOB] = 2
    _add("incomplete_ll_two_len2", Deflate().dynamic_block(ll, [0], lits(b"a") + [("L", EOB)]), "invalid",
         "invalid literal/lengths set", early=True, check=lambda h: _nz(h["ll"]) == {A: 2, EOB: 2})
    _add("single_eob_len2", Deflate().dynamic_block([0] * 256 + [2], [0], [("L", EOB)]), "invalid",
         "invalid literal/lengths set", early=True, check=lambda h: _nz(h["ll"]) == {EOB: 2})
    _add("single_dist_len2", Deflate().dynamic_block(ll_am, [2], [("L", A)] + match(3, 1) + [("L", EOB)]), "invalid",
         "invalid distances set", early=True, check=lambda h: h["dd"] == [2] and kraft(h["ll"]) == 32768)
    ll = [0] * 257
    ll[A] = ll[B] = 1
    _add("eob_len0", Deflate().dynamic_block(ll, [0], lits(b"ab")), "invalid", "missing end-of-block", early=True,
         check=lambda h: h["ll"][EOB] == 0 and kraft(h["ll"]) == 32768)
    for n in (287, 288):
        _add(f"hlit{n}", Deflate().dynamic_block(complete_lens(range(n), n), [0], [("L", EOB)]), "invalid",
             "too many length or distance symbols", early=True, check=lambda h, n=n: h["hlit"] == n and h["hdist"] == 1)
    for n in (31, 32):
        _add(f"hdist{n}", Deflate().dynamic_block(_ll([A, EOB]), complete_lens(range(n), n), [("L", EOB)]), "invalid",
             "too many length or distance symbols", early=True, check=lambda h, n=n: h["hdist"] == n and h["hlit"] == 257)
    _add("rep16_first", Deflate().dynamic_block(ll_ab, [0], [("X", 0, 32)], cl_lens=CL_RLE, cl_syms=[(16, 0)] + cl_zeros(94)),
         "invalid", "invalid bit length repeat", early=True, check=lambda h: h["bad"] == "16 first")
    _add("repeat_past_end", Deflate().dynamic_block(ll_ab, [0], [("X", 0, 32)], cl_lens=CL_RLE,
                                                    cl_syms=cl_zeros(97) + [2, 2] + cl_zeros(157) + [2, 2, (17, 0)]),
         "invalid", "invalid bit length repeat", early=True,
         check=lambda h: h["bad"] == "repeat past the end" and h["ops"][-1] == (17, 258, 3) and h["hlit"] + h["hdist"] == 259)
    _add("unused_code_single_dist", Deflate().dynamic_block(ll_am, [1], [("L", 257), ("C", 1, 1), ("X", 0, 16)]), "invalid",
         "invalid distance code", early=True, check=lambda h: h["dd"] == [1])
    _add("length_without_dist_codes", Deflate().dynamic_block(ll_am, [0], [("L", 257), ("X", 0, 16)]), "invalid",
         "invalid distance code", early=True, check=lambda h: h["dd"] == [0] and h["ll"][257] != 0)
    for s in (286, 287):
        _add(f"fixed_sym{s}", Deflate().fixed_block([("L", s), ("X", 0, 16)], True), "invalid", "invalid literal/length code",
             early=True)
    for s in (30, 31):
        _add(f"fixed_dist{s}", Deflate().fixed_block(lits(b"a") + [("L", 257), ("D", s), ("X", 0, 16)], True), "invalid",
             "invalid distance code")
    _add("btype3", Deflate().bits(1, 1).bits(3, 2).bits(0, 29), "invalid", "invalid block type", early=True)
    _add("stored_nlen_mismatch", Deflate().stored(b"abcde", True, nlen=0xFFFA ^ 0x0100), "invalid",
         "invalid stored block lengths", early=True)
    for n in (1, 16384, 32767):
        _add(f"dist_too_far_after_stored{n}", Deflate().stored(hist[:n], False).fixed_block(match(3, n + 1) + [("L", EOB)], True),
             "invalid", "invalid distance too far back")
        _add(f"dist_too_far_after_literals{n}", Deflate().fixed_block(lits(hist[:n]) + match(3, n + 1) + [("L", EOB)], True),
             "invalid", "invalid distance too far back")
    _add("wrong_adler32", hello, "invalid", "incorrect data check")
    WRAPPED["wrong_adler32"] = b"\x78\x9c" + hello + struct.pack(">I", zlib.adler32(b"hello") ^ 1)


_build()
# the paths a case runs on besides the stream kernel: the indexed kernels take one sw block of
# at most 32768 bytes from bit 16; the Adler-32 belongs to the stream mode alone
STREAM_ONLY = {"wrong_adler32"} | {n for n, _, k in CASES if k == "valid" and len(expected(n)) > 32768}
# stored history, then the match: also decoded as two chained sw blocks (name -> history bytes)
TWO_BLOCK = {n: 32768 for n in ("stored32768_dist32768", "stored32768_dist32767", "stored32768_dist32507")}

# The contract (include/dmx.h, deflate_decompress): the status of every invalid case, the same
# from the host decoder and from the GPU stream kernel.
STATUS = {
    **{n: "E_HUFAMB" for n in ("oversubscribed_ll", "oversubscribed_dist", "oversubscribed_cl", "incomplete_cl", "empty_cl",
                               "incomplete_ll_two_len2", "single_eob_len2", "single_dist_len2")},
    **{n: "E_ZINV" for n in ("eob_len0", "hlit287", "hlit288", "hdist31", "hdist32", "rep16_first", "repeat_past_end")},
    **{n: "E_HUFINV" for n in ("unused_code_single_dist", "length_without_dist_codes", "fixed_dist30", "fixed_dist31")},
    **{n: "E_HUFVAL" for n in ("fixed_sym286", "fixed_sym287")},
    "btype3": "E_ZBTYPE",
    "stored_nlen_mismatch": "E_ZNLEN",
    **{f"dist_too_far_after_{f}{n}": "E_HUFDIS" for f in ("stored", "literals") for n in (1, 16384, 32767)},
    "wrong_adler32": "E_ZADL32",
}
assert set(STATUS) == {n for n, _, k in CASES if k == "invalid"}
