"""Inputs of the seek-point index from the one-pass decode (test_zindex_gpu_api.py,
test_gpu_zindex_from_parallel.py) beyond those of inflate_parallel_inputs.py and
inflate_parallel_dev_inputs.py.  Built once per process.

sync3001: the first 300 000 bytes of the text as a zlib-6 stream with a sync flush every 3 001
bytes.  3 001 is odd, so the chunks' output offsets -- the sources of the windows -- take every residue
mod 16, and at span 1 several points lie in the first 32 768 bytes: windows with a zero prefix.

high16: 1 MiB of bytes drawn uniformly from 0xF0 .. 0xFF at zlib level 6: every byte is large, so the
Adler sums of a 64 KiB piece are near their bounds, and at span 262 144 a point is four to five
pieces."""
import numpy as np

import inflate_parallel_inputs as I

_cache = {}


def sync3001_stream():
    """(zlib stream, data)"""
    if "sync" not in _cache:
        t = I.text()[:300_000]
        _cache["sync"] = (I.deflate(t, 6, 15, flush_every=3001), t)
    return _cache["sync"]


def high16_stream():
    """(zlib stream, data)"""
    if "high" not in _cache:
        rng = np.random.default_rng(0xF0F0)
        data = (rng.integers(0, 16, size=1 << 20, dtype=np.uint8) | 0xF0).astype(np.uint8).tobytes()
        _cache["high"] = (I.deflate(data, 6, 15), data)
    return _cache["high"]


def twin(chunks, data, span):
    """dmx_zindex_from_chunks_host on a plan's live chunks and the decoded bytes: (return code,
    points, adlers, windows) as numpy arrays (None after an error)"""
    import ctypes

    import deflate_compression_amd as D
    vp = ctypes.c_void_p
    ch = np.ascontiguousarray(chunks, dtype=D.PCHUNK_DTYPE)
    p, a, w, n = vp(0), vp(0), vp(0), ctypes.c_uint32(0)
    r = D.lib().dmx_zindex_from_chunks_host(vp(ch.ctypes.data), len(ch), data, len(data), span, ctypes.byref(p), ctypes.byref(a),
                                            ctypes.byref(w), ctypes.byref(n))
    if r:
        assert (p.value, a.value, w.value, n.value) == (None, None, None, 0)
        return r, None, None, None
    try:
        k = n.value
        points = np.frombuffer(ctypes.string_at(p, 32 * k), dtype=D.PCHUNK_DTYPE).copy()
        adlers = np.frombuffer(ctypes.string_at(a, 4 * k), dtype=np.uint32).copy()
        windows = np.frombuffer(ctypes.string_at(w, 32768 * k), dtype=np.uint8).reshape(k, 32768).copy()
    finally:
        libc = ctypes.CDLL(None)
        libc.free.argtypes = [vp]
        libc.free.restype = None
        for q in (p, a, w):
            libc.free(q)
    return 0, points, adlers, windows


def streams():
    """[(name, stream, fmt, data, chunk_bytes)]: every stream the index is built of in both test files"""
    if "all" not in _cache:
        import inflate_parallel_dev_inputs as P
        out = [(name, z, fmt, data, 4096) for name, z, fmt, data in I.round_trip_inputs()]
        out.append(("sync3001", sync3001_stream()[0], "zlib", sync3001_stream()[1], 1024))
        out.append(("high16", high16_stream()[0], "zlib", high16_stream()[1], 4096))
        out.append(("run", P.run_stream()[0], "zlib", P.run_stream()[1], 1024))
        out.append(("edge", I.window_edge_stream()[0], "zlib", I.window_edge_stream()[1], 1024))
        _cache["all"] = out
    return _cache["all"]
