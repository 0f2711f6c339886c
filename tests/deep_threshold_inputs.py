"""Two full blocks on either side of DMX_F_DEEP's threshold: the block is deep
when 4 D < samples, D = the distinct 13-bit buckets of the trigrams at the sampled positions
(p < n - 2 with p mod 2048 < 256: 4 096 in a full block).  `pair()` returns (deep, shallow):
the same block up to one byte, with D = 1023 (4 D = samples - 4: deep) and D = 1024
(4 D = samples: not deep).  Shared by tests/test_deep_threshold.py (the oracle's verdict, no GPU)
and tests/test_gpu_k1_housekeeping.py (the match kernel's)."""
import functools

import numpy as np

B = 32768
SAMPLES = 4096


def distinct_buckets(a: np.ndarray) -> int:
    """D of a block, stated independently of the oracle (as tests/test_deep.py's rule)."""
    x = a.astype(np.uint64)
    p = np.arange(max(a.size - 2, 0))
    p = p[(p % 2048) < 256]
    t = x[p] | (x[p + 1] << np.uint64(8)) | (x[p + 2] << np.uint64(16))
    h = ((t * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(19)
    return int(np.unique(h).size)


@functools.lru_cache(maxsize=None)
def pair():
    """Ten-letter noise (D just under 1 000), then D raised one step at a time: a fresh byte
    value inside a sampled run changes up to three sampled trigrams.  Any increase is taken
    while D stays below 1015, from there only increases of exactly 1, so that D = 1023 and
    D = 1024 are both met and differ in the last byte written."""
    a = np.random.default_rng(7).integers(97, 107, B, dtype=np.uint8)
    d = distinct_buckets(a)
    assert d < 1015
    deep = None
    for k in range(16 * 125):
        r, i = k % 16, k // 16
        pos = r * 2048 + 5 + 2 * i
        old = a[pos]
        a[pos] = 150 + k % 90
        nd = distinct_buckets(a)
        ok = (nd == d + 1) if d >= 1015 else (d < nd <= 1024)
        if not ok:
            a[pos] = old
            continue
        d = nd
        if d == 1023:
            deep = a.copy()
        if d == 1024:
            break
    assert deep is not None and d == 1024
    shallow = a.copy()
    assert int((deep != shallow).sum()) == 1
    return deep.tobytes(), shallow.tobytes()
