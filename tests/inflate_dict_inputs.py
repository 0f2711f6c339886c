"""Streams with preset dictionaries for test_inflate_dict_api.py (the host decoder) and
test_gpu_inflate_dict.py (dmx_inflate_batch_dict_async): dictionaries of every length at which the
priming or the DICTID takes another path, streams that zlib writes against them (zlib with FDICT and
raw) and crafted first tokens (deflate_craft).  zlib is the reference: Case.want and Case.status come
from zlib.decompressobj(wbits, zdict=d) on the same bytes, never from the code under test.
"""
import struct
import zlib

import deflate_compression_amd as D
import deflate_craft as C

E = {k: -v for k, v in D.E.items()}
AUTO, ZLIB, GZIP, RAW = D.DMX_BATCH_AUTO, D.DMX_BATCH_ZLIB, D.DMX_BATCH_GZIP, D.DMX_BATCH_RAW
FMT_NAME = {AUTO: "auto", ZLIB: "zlib", GZIP: "gzip", RAW: "raw"}
DLENS = [0, 1, 15, 16, 17, 257, 258, 32767, 32768, 32769, 40000]

_dict_cache = {}


def dictionary(n, seed=11):
    """n bytes of text; the longer ones share no prefix with the shorter (another seed per length)"""
    if (n, seed) not in _dict_cache:
        _dict_cache[(n, seed)] = D.gen_text(n, seed + n).tobytes() if n else b""
    return _dict_cache[(n, seed)]


def payload(d, seed):
    """about 2 KB that repeats the dictionary's ends, so a parse against it reaches into it"""
    mid = D.gen_text(1500, seed).tobytes()
    return d[-200:] + mid + d[:300] + mid[:100] + d[-40:]


def deflate(data, d, wbits, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, zdict=d) if d is not None else zlib.compressobj(level, zlib.DEFLATED, wbits)
    return c.compress(data) + c.flush()


def fdict_wrap(raw, d, data):
    """a zlib stream with FDICT around raw DEFLATE data: 78 BB, DICTID, the data, Adler-32 of the output"""
    return b"\x78\xbb" + struct.pack(">I", zlib.adler32(d)) + raw + struct.pack(">I", zlib.adler32(data))


def zlib_says(z, d, wbits):
    """(bytes, in_used) from zlib.decompressobj(wbits, zdict=d), or None where zlib refuses the stream"""
    o = zlib.decompressobj(wbits, zdict=d) if d is not None else zlib.decompressobj(wbits)
    try:
        out = o.decompress(z)
    except zlib.error:
        return None
    if not o.eof:
        return None
    return out, len(z) - len(o.unused_data)


class Case:
    """One stream: its bytes, its framing (ZLIB / GZIP / RAW as it decodes; `fmt` the flag it is given),
    its dictionary (None: none), what zlib makes of it (want, used) or the status the contract names."""

    def __init__(self, name, z, fmt, d, status=0, ask=None):
        self.name, self.z, self.fmt, self.d, self.status = name, z, fmt, d, status
        self.ask = fmt if ask is None else ask
        wbits = {ZLIB: 15, GZIP: 31, RAW: -15}[fmt]
        # a zlib stream without FDICT and a gzip member ignore the dictionary; zlib itself wants none there
        takes = d is not None and (fmt == RAW or (fmt == ZLIB and len(z) > 1 and z[1] & 0x20))
        says = zlib_says(z, d if takes else None, wbits)
        if status:
            assert says is None, name + ": zlib accepts a stream the case calls bad"
            self.want, self.used = None, 0
        else:
            assert says is not None, name + ": zlib refuses a stream the case calls sound"
            self.want, self.used = says


def raw_match(length, dist, tail=b"xyz"):
    """a final fixed-code block: one match as the first token, then a few literals"""
    return C.Deflate().fixed_block(C.match(length, dist) + C.lits(tail) + [("L", 256)], True).getvalue()


_cases = []


def written_cases():
    """every dictionary length, zlib with FDICT and raw, as zlib writes them"""
    out = []
    for n in DLENS:
        d = dictionary(n)
        data = payload(d, 100 + n)
        out.append(Case(f"zlib dlen {n}", deflate(data, d, 15), ZLIB, d))
        out.append(Case(f"raw dlen {n}", deflate(data, d, -15), RAW, d))
    return out


def crafted_cases():
    out = []
    for n in (3, 17, 258, 4097, 32768, 40000):
        d = dictionary(n)
        p = min(n, 32768)   # the primed bytes
        for name, raw in (("first primed byte", raw_match(258, p)), ("distance 1", raw_match(258, 1)),
                          ("distance 3", raw_match(258, 3)),
                          ("across a stored block", C.Deflate().stored(bytes(range(20)), False)
                           .fixed_block(C.match(258, 20 + min(p, 50)) + [("L", 256)], True).getvalue())):
            says = zlib_says(raw, d, -15)
            assert says is not None, (name, n)
            out.append(Case(f"raw {name} dlen {n}", raw, RAW, d))
            out.append(Case(f"fdict {name} dlen {n}", fdict_wrap(raw, d, says[0]), ZLIB, d))
        if p < 32768:
            far = raw_match(258, p + 1)
            out.append(Case(f"raw too far dlen {n}", far, RAW, d, E["E_HUFDIS"]))
            out.append(Case(f"fdict too far dlen {n}", fdict_wrap(far, d, b""), ZLIB, d, E["E_HUFDIS"]))
    # an empty dictionary named by FDICT (DICTID 1): zlib itself writes no FDICT for it
    raw = deflate(b"no history at all", None, -15)
    out.append(Case("fdict empty dictionary", fdict_wrap(raw, b"", b"no history at all"), ZLIB, b""))
    out.append(Case("raw too far empty dictionary", raw_match(10, 1), RAW, b"", E["E_HUFDIS"]))
    return out


def negative_cases():
    d = dictionary(300)
    other = dictionary(301)
    data = payload(d, 5)
    zf = deflate(data, d, 15)
    assert zf[1] & 0x20
    plain = deflate(data, None, 15)
    gz = deflate(data, None, 31)
    out = [Case("fdict without a dictionary", zf, ZLIB, None, E["E_ZPDICT"]),
           Case("fdict with another dictionary", zf, ZLIB, other, E["E_ZPDICT"]),
           Case("no fdict, a dictionary given", plain, ZLIB, d),
           Case("gzip under auto, a dictionary given", gz, GZIP, d, ask=AUTO),
           Case("raw first match at distance 1, no dictionary", raw_match(61, 1), RAW, None, E["E_HUFDIS"]),
           Case("no fdict, a distance before the output, a dictionary given",
                C.zlib_wrap(raw_match(61, 1)), ZLIB, d, E["E_HUFDIS"])]
    for cut in (2, 3, 4, 5):
        out.append(Case(f"fdict cut at {cut}", zf[:cut], ZLIB, d, E["E_ZHEAD"]))
        out.append(Case(f"fdict cut at {cut}, no dictionary", zf[:cut], ZLIB, None, E["E_ZHEAD"]))
    out.append(Case("fdict cut at 6", zf[:6], ZLIB, d, E["E_LEN"]))
    return out


def all_cases():
    if not _cases:
        _cases.extend(written_cases() + crafted_cases() + negative_cases())
    return _cases
