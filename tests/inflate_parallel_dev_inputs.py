"""Inputs of the device decode of one foreign stream (test_gpu_inflate_parallel.py,
test_inflate_parallel_dev_api.py) beyond those of inflate_parallel_inputs.py: a stream with one chunk
whose last 32 768 cells are all references to before its own start, and streams whose first match
reaches before the first output byte.  Built once per process."""
import zlib

import numpy as np

import deflate_craft as C
import inflate_parallel_inputs as I

_cache = {}
RUN_OFF = 40_000   # the output offset of the run block


def run_stream():
    """(zlib stream, data): 40 000 bytes of text in literal blocks of 2 000, then ONE dynamic block of
    (8, 32768) followed by 300 x (258, 8) -- 77 408 bytes that are all copies of 8 bytes from 32 768
    back, so in a chunk that begins at this block every cell is a reference to before the chunk, the
    last 32 768 included -- then 16 blocks of about 1 000 bytes of matches 32 768 and 30 000 back, which
    read the run across several chunk starts."""
    if "run" not in _cache:
        t = I.text()[:RUN_OFF]
        d = C.Deflate()
        out = bytearray()
        for i in range(0, len(t), 2000):
            toks = list(t[i:i + 2000])
            I._block(d, toks)
            I._apply(toks, out)
        toks = [(8, 32768)] + [(258, 8)] * 300
        I._block(d, toks)
        I._apply(toks, out)
        rng = np.random.default_rng(9)
        for rnd in range(16):
            toks, made = [], 0
            while made < 1000:
                n = int(rng.integers(3, 9))
                toks.append((n, 32768 if rnd % 2 == 0 else 30000))
                made += n
                if rng.integers(0, 4) == 0:
                    toks.append(int(rng.integers(97, 123)))
                    made += 1
            I._block(d, toks, final=rnd == 15)
            I._apply(toks, out)
        data = bytes(out)
        z = C.zlib_wrap(d.getvalue(), data)
        assert zlib.decompress(z) == data
        _cache["run"] = (z, data)
    return _cache["run"]


def too_far_streams():
    """[(name, zlib stream, output offset of the bad match)]: the first match of the block at that
    offset reaches before the first output byte -- in the stream's first block, and in a block 10 000
    bytes in, behind literal blocks of 2 000 (a later chunk at chunk_bytes 1 024, out_off < 32 768)."""
    if "far" not in _cache:
        out = []
        d = C.Deflate()
        I._block(d, [97, (3, 5), 98, 99], final=True)
        out.append(("first-block", C.zlib_wrap(d.getvalue(), b"a"), 0))
        t = I.text()[:10_000]
        d = C.Deflate()
        for i in range(0, len(t), 2000):
            I._block(d, list(t[i:i + 2000]))
        I._block(d, [(8, 20000)] + list(t[:500]), final=True)
        out.append(("later-chunk", C.zlib_wrap(d.getvalue(), t), 10_000))
        for _, z, _ in out:
            try:
                zlib.decompress(z)
                raise AssertionError("zlib accepts a distance before the first byte")
            except zlib.error:
                pass
        _cache["far"] = out
    return _cache["far"]
