#!/usr/bin/env python3
"""The numbers of profiles/zindex_gpu/README.md: the seek-point index from the one-pass decode
(dmx_zindex_from_parallel_async, inflate_parallel_indexed) on one foreign stream of 100 MB resident
in HBM -- the "rebuilt" table's 100 MB of gen_text as one zlib-6 stream at the default cut.

Method, as tools/inflate_parallel_bench.py: one warm-up, then `--calls` calls back to back between
two synchronisations, the best of `--runs` runs and their spread; every output is compared with the
input and the device index with the host twin's.  plan + decode + index and the index alone are the
async calls on buffers allocated once; inflate_parallel_indexed and inflate_parallel are the Python
calls themselves, with their synchronisation, allocations and, for the first, the copy of the index
to the host.  zindex_build + inflate_indexed, the host route to the same state, runs in the same
process, one call a run.  Then the reads: inflate_indexed and 4 096 random 4 KiB reads with the
device-built index and with the host-built one.  One JSON line.

    python tools/zindex_gpu_bench.py
    python tools/zindex_gpu_bench.py --only-parallel --tree ../parent     # inflate_parallel alone, of another checkout
    rocprofv3 --kernel-trace --stats -d out -- python tools/zindex_gpu_bench.py --profile
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

D = None   # deflate_compression_amd, of this tree or of --tree


def sync():
    torch.cuda.synchronize()


def runs_of(fn, calls, runs):
    """[seconds per call] of `runs` runs of `calls` calls between two synchronisations, behind one warm-up"""
    fn()
    sync()
    out = []
    for _ in range(runs):
        sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        out.append((time.perf_counter() - t0) / calls)
    return out


def ms(v):
    return [round(1e3 * x, 3) for x in v]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mb", type=int, default=100)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--cut", type=int, default=0, help="chunk_bytes (0: the default)")
    ap.add_argument("--span", type=int, default=0, help="0: the default, 256 KiB")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tree", default=None, help="another checkout, built, whose package to time (the parent's, with --only-parallel)")
    ap.add_argument("--only-parallel", action="store_true", help="time inflate_parallel and nothing else")
    ap.add_argument("--profile", action="store_true", help="one plan + decode + index and nothing else (under rocprofv3)")
    a = ap.parse_args()
    global D
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import deflate_compression_amd
    D = deflate_compression_amd
    L = D.lib()
    n = a.mb * 1_000_000
    text = D.gen_text(n, 0xE5818)   # bench.py's C3 text
    data_t = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    z = zlib.compress(text.tobytes(), a.level)
    zt = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    row = {"row": f"text, zlib {a.level}", "cut": a.cut or 16384, "span": a.span or D.DMX_ZINDEX_DEF_SPAN, "stream_bytes": len(z),
           "out_bytes": n, "package": os.path.relpath(D.__file__)}
    info = {}
    assert torch.equal(D.inflate_parallel(zt, chunk_bytes=a.cut, info=info), data_t)
    row.update({k: info[k] for k in ("route", "nlive")})
    if a.only_parallel:
        row["inflate_parallel_ms"] = ms(runs_of(lambda: D.inflate_parallel(zt, chunk_bytes=a.cut), a.calls, a.runs))
        print(json.dumps(row), flush=True)
        return
    # the async chain on buffers allocated once
    nlive = info["nlive"]
    cap = L.dmx_zindex_points_bound(n, nlive, a.span)
    plan = torch.empty(L.dmx_inflate_parallel_plan_work(zt.numel(), a.cut), dtype=torch.uint8, device="cuda")
    work = torch.empty(info["work_len"], dtype=torch.uint8, device="cuda")
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    st = torch.empty(7, dtype=torch.int64, device="cuda")
    pts = torch.empty((cap, 4), dtype=torch.int64, device="cuda")
    adl = torch.empty(cap, dtype=torch.int32, device="cuda")
    win = torch.empty((cap, D.DMX_ZINDEX_WINDOW), dtype=torch.uint8, device="cuda")
    zwork = torch.empty(L.dmx_zindex_device_work(n, cap), dtype=torch.uint8, device="cuda")
    zst = torch.empty(5, dtype=torch.int64, device="cuda")

    def plan_decode():
        assert D.inflate_parallel_plan_async(zt, 0, a.cut, plan) == 0
        assert D.inflate_parallel_decode_async(zt, plan, nlive, dst, n, work, True, st) == 0

    def index_call():
        assert D.zindex_from_parallel_async(plan, st, dst, n, nlive, a.span, pts, adl, win, cap, zwork, zst) == 0

    def chain():
        plan_decode()
        index_call()

    chain()
    sync()
    if a.profile:
        return
    zrec = D.ZIndexStatus.from_buffer_copy(zst.cpu().numpy().tobytes())
    assert zrec.status == 0 and torch.equal(dst, data_t)
    row["npoints"], row["points_cap"] = zrec.npoints, cap
    row["index_bytes"] = zrec.npoints * (32 + 4 + D.DMX_ZINDEX_WINDOW)
    row["plan_decode_ms"] = ms(runs_of(plan_decode, a.calls, a.runs))
    row["index_ms"] = ms(runs_of(index_call, a.calls, a.runs))
    row["chain_ms"] = ms(runs_of(chain, a.calls, a.runs))
    # the Python calls
    out, ix = D.inflate_parallel_indexed(zt, chunk_bytes=a.cut, span=a.span)
    assert torch.equal(out, data_t) and ix.npoints == zrec.npoints
    row["inflate_parallel_indexed_ms"] = ms(runs_of(lambda: D.inflate_parallel_indexed(zt, chunk_bytes=a.cut, span=a.span), a.calls,
                                                    a.runs))
    row["inflate_parallel_ms"] = ms(runs_of(lambda: D.inflate_parallel(zt, chunk_bytes=a.cut), a.calls, a.runs))
    # the host route to the same state: index on the host, then the first decode
    hx = None

    def host_first_read():
        nonlocal hx
        hx = D.zindex_build(z, span=a.span)
        return D.inflate_indexed(zt, hx)

    assert torch.equal(host_first_read(), data_t)
    h = []
    for _ in range(a.runs):
        h += runs_of(host_first_read, 1, 1)
    row["zindex_build_first_read_ms"] = ms(h)
    row["first_read_ahead_in_every_run"] = bool(max(row["inflate_parallel_indexed_ms"]) < min(row["zindex_build_first_read_ms"]))
    # the device index is the host twin's, and both indexes read alike
    import ctypes
    chunks, _ = D.inflate_parallel_plan_host(z, chunk_bytes=a.cut)
    vp = ctypes.c_void_p
    tp, ta, tw, tn = vp(0), vp(0), vp(0), ctypes.c_uint32(0)
    assert L.dmx_zindex_from_chunks_host(vp(chunks.ctypes.data), len(chunks), vp(text.ctypes.data), n, a.span, ctypes.byref(tp),
                                         ctypes.byref(ta), ctypes.byref(tw), ctypes.byref(tn)) == 0
    assert tn.value == ix.npoints and ctypes.string_at(tp, 32 * tn.value) == ix.points.tobytes()
    assert ctypes.string_at(ta, 4 * tn.value) == ix.adlers.tobytes()
    assert ctypes.string_at(tw, D.DMX_ZINDEX_WINDOW * tn.value) == ix.windows.tobytes()
    row["equals_host_twin"] = True
    row["host_npoints"] = hx.npoints
    rng = np.random.default_rng(4096)
    ranges = np.stack([rng.integers(0, n - 4096, size=4096), np.full(4096, 4096)], axis=1)
    for tag, x in (("device", ix), ("host", hx)):
        assert torch.equal(D.inflate_indexed(zt, x), data_t)
        got, offs = D.zindex_read_ranges(zt, x, ranges)
        q = 1234
        assert torch.equal(got[offs[q]:offs[q + 1]], data_t[ranges[q, 0]:ranges[q, 0] + 4096])
        row[f"inflate_indexed_{tag}_ms"] = ms(runs_of(lambda: D.inflate_indexed(zt, x), a.calls, a.runs))
        row[f"reads_4096x4k_{tag}_ms"] = ms(runs_of(lambda: D.zindex_read_ranges(zt, x, ranges), a.calls, a.runs))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
