"""Inputs of test_refill_inputs.py / test_gpu_refill.py: streams whose tokens all have one size
that divides 32, and a CPU model of where the device reader refills on them.

The reader of csrc/dmx_inflate_dev.hip keeps bc bits in a 64-bit buffer and adds a 32-bit word
whenever bc <= 32 at one of two places of the symbol run (csrc/dmx_isym.inc): at a token's start,
and between a length (with its extra bits) and its distance.  Everything else refills through
ib_refill in compiled code.  After any such place bc is in (32, 64] and congruent to minus the bit
position, so the reader has no memory: a refill happens at the first of these places behind every
32-bit boundary of the stream (bit positions counted from the 4-byte aligned address at or below
the stream's first byte).  Tokens of T bits, T dividing 32, keep their offset mod T, so where a
boundary falls inside one token's length-to-distance gap it falls there in all of them: a stretch
whose every refill is the mid-token one.  Before the fix that refill did not rotate the reader's
two 64-word stream segments (vcur = words wb .. wb + 63, vnxt = the next 64), so wi - wb grew with
the stretch; from 128 on v_readlane's lane select wraps and the reader gets words it has consumed.

    parse(raw, bit0)        the tokens of a raw DEFLATE stream, by block (no output is made)
    refill_model(...)       longest run of mid-token refills and the largest wi - wb one sees
    equal_token_block(...)  a dynamic block of tokens that all have the same number of bits
    crafted_inputs()        [Input]: the geometries, starving and as controls
    zlib_inputs()           [Input]: zlib's own streams of constant input
    dict_inputs()           raw streams whose first matches reach into a preset dictionary
    cut_inputs()            streams cut inside a block whose all-zero code decodes for ever

Plain Python on tests/deflate_craft.py; built once per process; deterministic.
"""
import zlib
from collections import namedtuple

import numpy as np

import deflate_craft as C
import inflate_parallel_inputs as I

EOB = 256
NTOK = 5000          # tokens of a crafted block: 312 words at 2 bits a token
TAIL_WORDS = 192     # the run rotates while wb <= wfast - 192 (isym_run's wrl)

CRAFTED_NAMES = ["t2-zero-starving", "t2-zero-control", "t2-nolit-starving", "t2-nolit-control", "t4-starving", "t4-control",
                 "t8-starving", "t8-control", "t16-starving", "t16-control", "t3", "t6", "t2-zero-at-end", "t4-at-end",
                 "t2-zero-then-text", "t16-far-starving"]
ZLIB_NAMES = ["zeros-768k", "zeros-1m", "zeros-5m", "A-5m", "zeros-16m", "zeros-1m-gzip", "zeros-1m-raw"]

Input = namedtuple("Input", "name z fmt data kind T")   # kind: "starving" | "control" | "short" | "text"
_cache = {}


# ------------------------------------------------------------------------------------------
# Token positions
# ------------------------------------------------------------------------------------------
def _table(lens):
    """(list indexed by the next maxbits stream bits -> symbol << 4 | code length, mask)"""
    codes = C.canonical(lens)
    mb = max((n for n in lens if n), default=1)
    t = np.zeros(1 << mb, dtype=np.int32)
    for s, (c, n) in codes.items():
        r = int(format(c, f"0{n}b")[::-1], 2)   # codes go out MSB-first: the stream holds them reversed
        t[r::1 << n] = (s << 4) | n
    return t.tolist(), (1 << mb) - 1


_FIXED = None


def parse(raw, bit0=0):
    """The blocks of the raw DEFLATE stream that starts at bit bit0 of `raw`: a list of
    (header bit, end bit, tokens), tokens a list of (start bit, bit behind the length and its extra
    bits, end bit) -- a literal and the end-of-block code have the last two equal; a stored block
    has tokens None and its end behind its bytes.  Positions are bits of `raw`."""
    global _FIXED
    z = bytes(raw) + bytes(16)
    pos = bit0

    def bits(n):
        nonlocal pos
        v = (int.from_bytes(z[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    blocks = []
    last = False
    while not last:
        head = pos
        assert pos < 8 * len(raw), "no final block"
        last = bits(1) == 1
        bt = bits(2)
        if bt == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            assert bits(16) == n ^ 0xFFFF
            pos += 8 * n
            blocks.append((head, pos, None))
            continue
        assert bt != 3
        if bt == 1:
            if _FIXED is None:
                _FIXED = (_table(C.FIXED_LL), _table(C.FIXED_D))
            (lt, lm), (dt, dm) = _FIXED
        else:
            nl, nd, nc = bits(5) + 257, bits(5) + 1, bits(4) + 4
            cl = [0] * 19
            for k in range(nc):
                cl[C.CL_ORDER[k]] = bits(3)
            ct, cm = _table(cl)
            lens = []
            while len(lens) < nl + nd:
                e = ct[(int.from_bytes(z[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & cm]
                assert e & 15
                pos += e & 15
                s = e >> 4
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + bits(2))
                elif s == 17:
                    lens += [0] * (3 + bits(3))
                else:
                    lens += [0] * (11 + bits(7))
            assert len(lens) == nl + nd
            (lt, lm), (dt, dm) = _table(lens[:nl]), _table(lens[nl:])
        toks = []
        add = toks.append
        frm = int.from_bytes
        lext, dext = C.LEXT, C.DEXT
        while True:
            w = frm(z[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)
            e = lt[w & lm]
            n = e & 15
            assert n, "no literal/length code"
            s = e >> 4
            if s <= 256:
                add((pos, pos + n, pos + n))
                pos += n
                if s == 256:
                    break
                continue
            a = n + lext[s - 257]
            e = dt[(w >> a) & dm]
            assert e & 15, "no distance code"
            end = a + (e & 15) + dext[e >> 4]
            add((pos, pos + a, pos + end))
            pos += end
        blocks.append((head, pos, toks))
    return blocks


# ------------------------------------------------------------------------------------------
# The reader's refills
# ------------------------------------------------------------------------------------------
Refills = namedtuple("Refills", "run span tail_mid")


def refill_model(raw, bit0=0, lo=0, fixed=False):
    """The device reader on the raw stream at bit bit0 of `raw`, whose first byte lies lo bytes
    above a 4-byte aligned address.  Returns (run, span, tail_mid): the longest run of consecutive
    refills that all fall between a length and its distance, in words; the largest wi - wb such a
    refill reads at -- under the parent's rule (that refill never rotates; every other one rotates
    once when wi - wb >= 64), or with fixed=True under the rule that it rotates as well; and how
    many of them fall where the run may not rotate itself (wb > wfast - 192) and hands over."""
    off = 8 * lo
    wfast = (lo + len(raw)) >> 2
    wrl = wfast - TAIL_WORDS
    st = {"wb": 0, "word": 0, "run": 0, "best": 0, "span": 0, "tail": 0}

    def seek(p):    # ib_seek loads the word that holds p; the block header behind it refills at once
        st["word"] = (p + off) >> 5
        st["wb"] = st["word"] & ~63
        if st["word"] + 1 - st["wb"] >= 64:
            st["wb"] += 64
        st["run"] = 0

    seek(bit0)

    def other(p):   # every word boundary up to p is refilled by code that rotates
        w = (p + off) >> 5
        while st["word"] < w:
            st["word"] += 1
            if st["word"] + 1 - st["wb"] >= 64:
                st["wb"] += 64
            st["run"] = 0

    def mid(p):     # at most one boundary lies inside a token
        w = (p + off) >> 5
        if st["word"] < w:
            assert st["word"] + 1 == w
            st["word"] = w
            k = w + 1 - st["wb"]    # the word loaded is the one behind the word that holds p
            st["span"] = max(st["span"], k)
            if st["wb"] > wrl:
                st["tail"] += 1
            if fixed and k >= 64:
                st["wb"] += 64
            st["run"] += 1
            st["best"] = max(st["best"], st["run"])

    for head, end, toks in parse(raw, bit0):
        if toks is None:   # a stored block: the reader seeks behind it
            other(head + 3)
            seek(end)
            continue
        for s, a, e in toks:
            other(s)
            if a != e:
                mid(a)
        other(end)
    return Refills(st["best"], st["span"], st["tail"])


def body_bit(z, fmt):
    """the bit of z at which the raw DEFLATE stream begins (no optional gzip fields here)"""
    return {"zlib": 16, "gzip": 80, "raw": 0}[fmt]


def model_of(inp, lo=0, fixed=False):
    return refill_model(inp.z, body_bit(inp.z, inp.fmt), lo, fixed)


# ------------------------------------------------------------------------------------------
# Crafted blocks
# ------------------------------------------------------------------------------------------
LITS = b"acgt"


def equal_token_block(d, lsyms, lbits, dsyms, dbits, ntok, rng, out, final=False, lits=0, zero=False, log=None, edge=0):
    """One dynamic block on the writer d: `lits` literals, then ntok matches that all take
    lbits + LEXT + dbits + DEXT bits -- a length symbol of lsyms (all with codes of lbits bits and
    the same extra bits) and a distance symbol of dsyms (likewise), extra bits drawn from rng.
    The literal/length code gives the length symbols half the code space (a quarter each at
    lbits = 2), the end of block a quarter and four literals a sixteenth each; zero=True is
    zlib's code for constant input instead, {0: 2, 256: 2, 285: 1}; and with lits < 0 there is no
    literal at all, {256: 1, 285: 1}.  A distance code that would be incomplete gets an unused
    1-bit code beside it (a single 1-bit code is legal as it is).  `out` (bytearray) is extended,
    `log` (a list) by every (length, distance).  edge: every edge-th match has the largest distance the
    symbols spell."""
    assert len(lsyms) << (15 - lbits) == 16384
    ll = [0] * (max(lsyms) + 1)
    if lits < 0:
        assert lsyms == [285] and lbits == 1
        ll[EOB] = 1
        alphabet = b""
    elif zero:
        ll[0] = ll[EOB] = 2
        alphabet = b"\0"
    else:
        ll[EOB] = 2
        for b in LITS:
            ll[b] = 4
        alphabet = LITS
    for s in lsyms:
        ll[s] = lbits
    assert C.kraft(ll) == 32768
    dd = [0] * (max(dsyms) + 1)
    for s in dsyms:
        dd[s] = dbits
    if C.kraft(dd) != 32768 and not (len(dsyms) == 1 and dbits == 1):
        filler = min(set(range(30)) - set(dsyms))
        dd[filler] = 1
        assert C.kraft(dd) == 32768
    lx, dx = C.LEXT[lsyms[0] - 257], C.DEXT[dsyms[0]]
    assert all(C.LEXT[s - 257] == lx for s in lsyms) and all(C.DEXT[s] == dx for s in dsyms)
    items = []
    for _ in range(max(lits, 0)):
        b = alphabet[int(rng.integers(0, len(alphabet)))]
        items.append(("L", b))
        out.append(b)
    for k in range(ntok):
        ls = lsyms[int(rng.integers(0, len(lsyms)))]
        ds = dsyms[int(rng.integers(0, len(dsyms)))]
        lv, dv = int(rng.integers(0, 1 << lx)), int(rng.integers(0, 1 << dx))
        if edge and k % edge == edge - 1:
            ds, dv = max(dsyms), (1 << dx) - 1
        length, dist = C.LBASE[ls - 257] + lv, C.DBASE[ds] + dv
        assert dist <= len(out)
        if log is not None:
            log.append((length, dist))
        items += [("L", ls), ("X", lv, lx), ("D", ds), ("X", dv, dx)]
        src = bytes(out[-dist:])
        out += (src * (length // dist + 1))[:length]
    items.append(("L", EOB))
    d.dynamic_block(ll, dd, items, cl_lens=I.CL_ALL, cl_syms=C.cl_rle(ll + dd), final=final)
    return lbits + lx + dbits + dx


# name: (T, length symbols, code bits, distance symbols, code bits, literals in front, zero)
GEOMETRY = {
    "t2-zero": (2, [285], 1, [0], 1, 1, True),          # zlib's own: 258 bytes at distance 1, two 1-bit codes
    "t2-nolit": (2, [285], 1, [0], 1, -1, False),       # {256: 1, 285: 1}: the history is a stored byte
    "t4": (4, [265], 1, [4, 5], 1, 8, False),           # 1 + 1 length bits, 1 + 1 distance bits: 5 .. 8 back
    "t8": (8, [269, 270], 2, [8], 1, 32, False),        # 2 + 2, 1 + 3: 17 .. 24 back
    "t16": (16, [277, 278], 2, [18, 19], 2, 1024, False),   # 2 + 4, 2 + 8: 513 .. 1024 back
    "t3": (3, [285], 1, [4], 1, 8, False),              # controls: the offset mod T moves against the words
    "t6": (6, [265], 1, [8], 1, 32, False),             # 1 + 1, 1 + 3
}
CONTROL_T = (3, 6)


def _prefix(d, ndyn, nfix):
    """empty blocks in front: ndyn dynamic ones (111 bits each) and nfix fixed ones (10 bits)"""
    for _ in range(ndyn):
        I._block(d, [])
    for _ in range(nfix):
        d.fixed_block([("L", EOB)], False)


def _crafted(name, ndyn, nfix, seed=11, tail="stored", far=False, log=None):
    """(raw stream, data) of geometry `name` with the given empty blocks in front of its block.  tail: "stored" puts
    1 KiB of stored bytes behind the block (its whole stretch lies where the run rotates itself),
    "none" ends the stream with the block (the stretch runs into the last 192 words), "text" a
    stored block and a block of text.  far: geometry of its own -- 32 768 stored bytes, then
    16-bit tokens of 258 bytes from 16 385 .. 32 768 back."""
    rng = np.random.default_rng(seed)
    d, out = C.Deflate(), bytearray()
    final = tail == "none"
    if far:
        hist = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
        d.stored(hist, False)
        out += hist
        _prefix(d, ndyn, nfix)
        T = equal_token_block(d, [285], 1, [28, 29], 2, NTOK, rng, out, final=final, log=log, edge=50)
        assert T == 16
    else:
        T, lsyms, lbits, dsyms, dbits, lits, zero = GEOMETRY[name]
        if lits < 0:
            d.stored(b"\x5a", False)
            out += b"\x5a"
        _prefix(d, ndyn, nfix)   # (behind the stored history, which ends on a byte boundary whatever is in front)
        assert equal_token_block(d, lsyms, lbits, dsyms, dbits, NTOK, rng, out, final=final, lits=lits, zero=zero) == T
    if tail != "none":
        junk = rng.integers(0, 256, 1024, dtype=np.uint8).tobytes()
        d.stored(junk, tail == "stored")
        out += junk
    if tail == "text":
        t = I.text()[:3000]
        I._block(d, list(t), final=True)
        out += t
    return d.getvalue(), bytes(out)


def _align(name, want_starving, base=(0, 0), **kw):
    """the first (ndyn, nfix) at or behind `base` for which the model calls the stream starving
    (a run of at least 256 words) or not (at most 2)"""
    for extra in range(8):
        for nd in range(extra + 1):
            ndyn, nfix = base[0] + nd, base[1] + extra - nd
            if want_starving is False and (ndyn, nfix) == base:
                continue
            raw, data = _crafted(name, ndyn, nfix, **kw)
            run = refill_model(raw, 0, 2).run   # as a zlib stream at an aligned address: 2 bytes in
            if (run >= 256) if want_starving else (run <= 2):
                return (ndyn, nfix), raw, data
    raise AssertionError(f"no alignment makes {name} " + ("starving" if want_starving else "a control"))


def crafted_inputs():
    """[Input]: each power-of-two geometry starving and, behind one more empty block, as a control;
    T = 3 and 6 as controls; the starving T = 2 stretch at the stream's very end, in front of a
    stored block and text, and the 16-bit tokens that reach 32 768 back."""
    if "crafted" not in _cache:
        out = []

        def add(nm, raw, data, kind, T):
            out.append(Input(nm, C.zlib_wrap(raw, data), "zlib", data, kind, T))

        for name, g in GEOMETRY.items():
            T = g[0]
            if T in CONTROL_T:
                raw, data = _crafted(name, 0, 0)
                add(name, raw, data, "control", T)
                continue
            base, raw, data = _align(name, True)
            add(name + "-starving", raw, data, "starving", T)
            _, raw, data = _align(name, False, base)
            add(name + "-control", raw, data, "control", T)
        base, raw, data = _align("t2-zero", True, tail="none", seed=12)
        add("t2-zero-at-end", raw, data, "starving", 2)
        base, raw, data = _align("t4", True, tail="none", seed=13)
        add("t4-at-end", raw, data, "starving", 4)
        base, raw, data = _align("t2-zero", True, tail="text", seed=14)
        add("t2-zero-then-text", raw, data, "starving", 2)
        base, raw, data = _align("far", True, far=True, seed=15)
        add("t16-far-starving", raw, data, "starving", 16)
        _cache["far-matches"] = []
        assert _crafted("far", *base, far=True, seed=15, log=_cache["far-matches"])[0] == raw
        assert [i.name for i in out] == CRAFTED_NAMES
        _cache["crafted"] = out
    return _cache["crafted"]


def far_matches():
    """[(length, distance)] of the matches of t16-far-starving"""
    crafted_inputs()
    return _cache["far-matches"]


def zlib_inputs():
    """[Input]: zlib's own level-6 streams of constant input.  "starving" where the model finds
    runs of 1 000 words and more, "short" for the two whose single block ends before 256 (768 KiB:
    about 190 words, 1 MiB: about 254) -- still past the 128 from which a read goes wrong."""
    if "zlib" not in _cache:
        out = []
        for nm, data, kind in (("zeros-768k", bytes(768 << 10), "short"), ("zeros-1m", bytes(1 << 20), "short"),
                               ("zeros-5m", bytes(5 << 20), "starving"), ("A-5m", b"A" * (5 << 20), "starving"),
                               ("zeros-16m", bytes(16 << 20), "starving")):
            out.append(Input(nm, zlib.compress(data, 6), "zlib", data, kind, 2))
        one = bytes(1 << 20)
        out.append(Input("zeros-1m-gzip", I.deflate(one, 6, 31), "gzip", one, "short", 2))
        out.append(Input("zeros-1m-raw", I.deflate(one, 6, -15), "raw", one, "short", 2))
        assert [i.name for i in out] == ZLIB_NAMES
        _cache["zlib"] = out
    return _cache["zlib"]


def text_stream():
    """(zlib stream, data): 20 000 bytes of text at level 6, the good neighbour of the batches"""
    t = I.text()[:20_000]
    return zlib.compress(t, 6), t


# ------------------------------------------------------------------------------------------
# Raw streams whose first matches reach into a preset dictionary
# ------------------------------------------------------------------------------------------
def dict_inputs():
    """(zdict, [(name, raw stream, data)]): the starving 2-, 4- and 16-bit geometries as raw
    streams without their literals -- the history of the first matches is the dictionary's end."""
    if "dict" not in _cache:
        rng = np.random.default_rng(31)
        zdict = bytes(LITS[int(v)] for v in rng.integers(0, 4, 2048))
        out = []
        for name in ("t2-zero", "t4", "t16"):
            T, lsyms, lbits, dsyms, dbits, _, zero = GEOMETRY[name]
            found = None
            for extra in range(8):
                for nd in range(extra + 1):
                    r2 = np.random.default_rng(32)
                    d, hist = C.Deflate(), bytearray(zdict)
                    _prefix(d, nd, extra - nd)
                    equal_token_block(d, lsyms, lbits, dsyms, dbits, NTOK, r2, hist, lits=0, zero=zero)
                    junk = r2.integers(0, 256, 1024, dtype=np.uint8).tobytes()
                    d.stored(junk, True)
                    hist += junk
                    if refill_model(d.getvalue(), 0, 0).run >= 256:
                        found = (name + "-dict", d.getvalue(), bytes(hist[len(zdict):]))
                        break
                if found:
                    break
            assert found, name
            out.append(found)
        _cache["dict"] = (zdict, out)
    return _cache["dict"]


# ------------------------------------------------------------------------------------------
# Streams cut inside a block: what do the zeros behind the cut spell?
# ------------------------------------------------------------------------------------------
def cut_inputs():
    """[(name, cut zlib stream)]: dynamic blocks with explicit code lengths, cut in the middle of
    their tokens, whose all-zero code is (a) a literal, (b) a length, with an all-zero distance
    code, (c) the end of block; and the level-6 text stream cut at 10 places inside block bodies.
    Behind the cut the reader hands out zeros: (a) and (b) decode them as output for ever."""
    if "cut" not in _cache:
        out = []
        A, B = 97, 98
        # (a) literal 'a' is the 1-bit code 0
        ll = [0] * 258
        ll[A], ll[B], ll[EOB], ll[257] = 1, 2, 3, 3
        items = C.lits(b"ab" * 40) + C.match(3, 1) * 20 + C.lits(b"ba" * 40) + [("L", EOB)]
        raw = C.Deflate().dynamic_block(ll, [1], items).getvalue()
        assert C.canonical(ll)[A] == (0, 1)
        out.append(("zero-is-literal", raw))
        # (b) length 258 is the 1-bit code 0, distance 1 the 1-bit code 0 (zlib's zero block)
        ll = [0] * 286
        ll[0], ll[EOB], ll[285] = 2, 2, 1
        items = [("L", 0)] + C.match(258, 1) * 300 + [("L", EOB)]
        raw = C.Deflate().dynamic_block(ll, [1], items).getvalue()
        assert C.canonical(ll)[285] == (0, 1) and C.canonical([1])[0] == (0, 1)
        out.append(("zero-is-length", raw))
        # (c) the end of block is the 1-bit code 0: the zeros end the block and go on as block headers
        ll = [0] * 258
        ll[A], ll[B], ll[EOB], ll[257] = 2, 3, 1, 3
        items = C.lits(b"ab" * 60) + C.match(3, 1) * 20 + C.lits(b"ba" * 20) + [("L", EOB)]
        raw = C.Deflate().dynamic_block(ll, [1], items).getvalue()
        assert C.canonical(ll)[EOB] == (0, 1)
        out.append(("zero-is-eob", raw))
        cuts = []
        for name, raw in out:
            blocks = parse(raw)
            toks = blocks[0][2]
            for frac in (0.3, 0.7):
                bit = toks[int(len(toks) * frac)][0]
                z = C.zlib_wrap(raw)
                cuts.append((f"{name}-{frac}", z[:2 + (bit + 7) // 8]))
        z, _ = text_stream()
        blocks = parse(z, 16)
        body = [(b[2][0][0], b[1]) for b in blocks if b[2]]
        first, end = body[0][0], body[-1][1]
        for j in range(10):
            bit = first + (end - first) * (2 * j + 1) // 20
            assert any(lo < bit < hi for lo, hi in body)
            cuts.append((f"text-cut{j}", z[:bit // 8]))
        _cache["cut"] = cuts
    return _cache["cut"]
