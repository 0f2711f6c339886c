"""Inputs of test_inflate_parallel_api.py (one foreign stream cut at true block starts):
streams of Python's zlib over about 1.5 MiB of synthetic text, hand-built streams whose matches
reach the window's edge across chunk starts (zlib's own encoder never emits a distance above
32 506), streams without a dynamic block, and stored blocks that carry a whole DEFLATE stream as
their payload -- block starts that are not blocks of the stream.  Built once per process."""
import struct
import zlib

import numpy as np

import deflate_compression_amd as D
import deflate_craft as C

TEXT_BYTES = 1_500_000
CHUNKS = (1024, 4096, 65536)
_cache = {}


def deflate(data, level=6, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, full=False):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = []
    for i in range(0, len(data), flush_every):
        out.append(c.compress(data[i:i + flush_every]))
        out.append(c.flush(zlib.Z_FULL_FLUSH if full else zlib.Z_SYNC_FLUSH))
    return b"".join(out) + c.flush()


def text():
    if "text" not in _cache:
        _cache["text"] = D.gen_text(TEXT_BYTES, 7).tobytes()
    return _cache["text"]


def round_trip_inputs():
    """[(name, stream, fmt, data)]: levels 1, 6, 9 as zlib, gzip and raw, and Z_SYNC_FLUSH every 3 000 bytes"""
    if "rt" not in _cache:
        t = text()
        out = []
        for level in (1, 6, 9):
            for fmt, wbits in (("zlib", 15), ("gzip", 31), ("raw", -15)):
                out.append((f"l{level}-{fmt}", deflate(t, level, wbits), fmt, t))
        out.append(("l6-zlib-sync3000", deflate(t, 6, 15, flush_every=3000), "zlib", t))
        _cache["rt"] = out
    return _cache["rt"]


def bits_of(z, bit, end_bit, tail=0, tail_bits=0):
    """bits [bit, end_bit) of z as a byte string that starts at bit 0, `tail` appended behind them"""
    lo, hi = bit >> 3, (end_bit + 7) >> 3
    v = int.from_bytes(z[lo:hi], "little") >> (bit & 7)
    n = end_bit - bit
    v = (v & ((1 << n) - 1)) | (tail << n)
    return v.to_bytes((n + tail_bits + 7) >> 3, "little")


def check_chunks(z, data, chunks, body_bit):
    """zlib's own verdict on a plan: the chunks tile the output, follow one another in the stream,
    and bits [bit, end_bit) of each, behind the 32 KiB of output in front of it and in front of an
    empty final block, are whole blocks that inflate to exactly that chunk's bytes."""
    assert len(chunks) >= 1 and int(chunks["bit"][0]) == body_bit and int(chunks["out_off"][0]) == 0
    off = 0
    for k in range(len(chunks)):
        bit, end, o, n = (int(chunks[f][k]) for f in ("bit", "end_bit", "out_off", "out_len"))
        assert o == off and end > bit, (k, o, off)
        if k + 1 < len(chunks):
            assert int(chunks["bit"][k + 1]) == end, k
        # BFINAL = 1, BTYPE = 01, the 7-bit end-of-block code: ten bits that end the stream here
        raw = bits_of(z, bit, end, tail=0b0000000_01_1, tail_bits=10)
        d = zlib.decompressobj(-15, zdict=data[max(0, o - 32768):o]) if o else zlib.decompressobj(-15)
        got = d.decompress(raw)
        assert d.eof and got == data[o:o + n], (k, bit, end, len(got), n)
        off += n
    assert off == len(data)


# ---- hand-built streams --------------------------------------------------------------------

# a complete code length code with a code for every symbol: 13 of 4 bits, 6 of 5 bits
CL_ALL = {**{s: 4 for s in range(13)}, **{s: 5 for s in range(13, 19)}}

def _block(d, tokens, final=False):
    """one dynamic block of `tokens` (a byte, or (length, distance)) with Huffman codes of its own"""
    items, fl, fd = [], {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            items.append(("L", t))
            fl[t] = fl.get(t, 0) + 1
        else:
            m = C.match(*t)
            items += m
            fl[m[0][1]] = fl.get(m[0][1], 0) + 1
            fd[m[2][1]] = fd.get(m[2][1], 0) + 1
    items.append(("L", 256))
    if len(fl) < 2:
        fl[0] = 1
    ll = C.huffman_lens(fl, max(fl) + 1)
    ll += [0] * (257 - len(ll))
    if len(fd) >= 2:
        dd = C.huffman_lens(fd, max(fd) + 1)
    else:   # no distance code, or a single code of length 1: the incomplete codes a decoder must take
        dd = [0] * (max(fd) + 1 if fd else 1)
        if fd:
            dd[-1] = 1
    d.dynamic_block(ll, dd, items, cl_lens=CL_ALL, cl_syms=C.cl_rle(ll + dd), final=final)


def _apply(tokens, out):
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, dist = t
            for _ in range(n):
                out.append(out[-dist])


def window_edge_stream():
    """(zlib stream, data): 40 000 bytes of text in literal blocks of 2 000 bytes, then blocks of
    1 000 bytes each made of matches exactly 32 768 back (12 blocks), exactly 32 767 back (12
    blocks), and again 32 768 back: every block is a few hundred compressed bytes, so at
    chunk_bytes 1 024 the chunks begin inside the match blocks, a chunk holds 2-3 KB of output, and
    every match reads across 10 or more chunk starts at the window's very edge."""
    if "edge" not in _cache:
        t = text()[:40_000]
        d = C.Deflate()
        out = bytearray()
        for i in range(0, len(t), 2000):
            toks = list(t[i:i + 2000])
            _block(d, toks)
            _apply(toks, out)
        rng = np.random.default_rng(5)
        for rnd, dist in enumerate([32768] * 12 + [32767] * 12 + [32768] * 6):
            toks, made = [], 0
            while made < 1000:
                n = int(rng.integers(3, 9))
                toks.append((n, dist))
                made += n
                if rng.integers(0, 4) == 0:
                    toks.append(int(rng.integers(97, 123)))
                    made += 1
            _block(d, toks, final=rnd == 29)
            _apply(toks, out)
        data = bytes(out)
        z = C.zlib_wrap(d.getvalue(), data)
        assert zlib.decompress(z) == data
        _cache["edge"] = (z, data)
    return _cache["edge"]


def stored_only_stream():
    t = text()[:50_000]
    d = C.Deflate()
    for i in range(0, len(t), 5000):
        d.stored(t[i:i + 5000], i + 5000 >= len(t))
    z = C.zlib_wrap(d.getvalue(), t)
    assert zlib.decompress(z) == t
    return z, t


def fixed_only_stream():
    t = text()[:30_000]
    z = deflate(t, 6, 15, zlib.Z_FIXED)
    return z, t


def false_candidate_stream(payload_bytes):
    """(zlib stream, data): a stored block whose payload is a complete raw DEFLATE stream of small
    dynamic blocks (a full flush every 300 bytes of text), then the real thing: text in dynamic
    blocks.  The payload's blocks are not blocks of this stream; chunks that begin inside it find them."""
    key = ("false", payload_bytes)
    if key not in _cache:
        t = text()
        inner, n = b"", 0
        while len(inner) < payload_bytes:   # the longest inner stream that fits
            n += 300
            cand = deflate(t[100_000:100_000 + n], 6, -15, flush_every=300, full=True)
            if len(cand) > payload_bytes:
                break
            inner = cand
        assert 0 < len(inner) <= 65535 and zlib.decompress(inner, -15)
        tail = t[:60_000]
        z = b"\x78\x9c" + C.Deflate().stored(inner, False).getvalue() + deflate(tail, 6, -15, flush_every=3000)
        data = inner + tail
        z += struct.pack(">I", zlib.adler32(data))
        assert zlib.decompress(z) == data
        _cache[key] = (z, data)
    return _cache[key]


def flip_stream():
    """(zlib stream, data, 200 single-bit flips of it): about 6 KB in small dynamic blocks, several chunks of 1 024"""
    if "flip" not in _cache:
        t = text()[:14_000]
        z = deflate(t, 6, 15, flush_every=1500)
        assert len(z) > 5 * 1024
        rng = np.random.default_rng(21)
        flips = []
        for _ in range(200):
            c = bytearray(z)
            c[int(rng.integers(2, len(c)))] ^= 1 << int(rng.integers(0, 8))
            flips.append(bytes(c))
        _cache["flip"] = (z, t, flips)
    return _cache["flip"]
