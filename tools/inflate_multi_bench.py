#!/usr/bin/env python3
"""The numbers of profiles/inflate_multi/README.md: one .gz file of many members resident in HBM,
decoded in one pass (inflate_parallel_multi: dmx_inflate_parallel_multi_plan_async + _decode_async),
beside what the library could do before.  Medians of `--runs` runs (10 at least) behind `--warmup`
warm-up runs, timed with HIP events around the calls; every output is compared with the input.

  a   one file of two 50 MB zlib-6 text members: the multi decode against the sum of
      inflate_parallel on each member alone
  b   25 000 members of 4 KiB pages: against inflate_batch given the true member boundaries and
      sizes (the floor: no search), and against the host loop of single-member decodes a user has
      without this call (timed on 1 000 members and scaled)
  c   inflate_parallel on the 100 MB zlib-6 text; with --tree PATH the package is imported from PATH
      (a checkout of the parent commit, built), so two runs compare the shared kernels

    python tools/inflate_multi_bench.py --only a,b
    python tools/inflate_multi_bench.py --only c [--tree ../parent]

One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import zlib

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="a,b,c")
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--tree", default=None)
ap.add_argument("--mb", type=int, default=50, help="a: MB per member; c: twice that")
ap.add_argument("--members", type=int, default=25_000)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

import deflate_compression_amd as D   # noqa: E402


def timed(fn):
    """{median_ms, min_ms, max_ms, runs} of fn() by HIP events"""
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(max(args.runs, 10)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3),
            "runs": len(out)}


def gz(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def emit(**kw):
    print(json.dumps(kw), flush=True)


def multi_pair(zt, out_len):
    """the async pair on buffers allocated once -> (fn, out, status tensor)"""
    L = D.lib()
    info = {}
    D.inflate_parallel_multi(zt, info=info)
    assert info["route"] == "parallel", info
    plan = torch.empty(L.dmx_inflate_parallel_multi_plan_work(zt.numel(), 0), dtype=torch.uint8, device="cuda")
    out = torch.empty(out_len, dtype=torch.uint8, device="cuda")
    mem = torch.empty(4 * info["nmembers"], dtype=torch.int64, device="cuda")
    work = torch.empty(info["work_len"], dtype=torch.uint8, device="cuda")
    st = torch.empty(8, dtype=torch.int64, device="cuda")

    def fn():
        assert D.inflate_parallel_multi_plan_async(zt, D.DMX_BATCH_GZIP, 0, plan) == 0
        assert D.inflate_parallel_multi_decode_async(zt, plan, info["nlive"], info["nmembers"], out, out_len, mem, work, True,
                                                     st) == 0
    return fn, out, st, info


def bench_a():
    t = D.gen_text(2 * args.mb * 1_000_000, 7)
    half = args.mb * 1_000_000
    tb = t.tobytes()
    za, zb = gz(tb[:half]), gz(tb[half:])
    want = dev(tb)
    zt, zta, ztb = dev(za + zb), dev(za), dev(zb)
    fn, out, st, info = multi_pair(zt, 2 * half)
    r = timed(fn)
    assert int(st[0].item()) & 0xFFFFFFFF == 0 and torch.equal(out, want)
    emit(case="a", what="multi plan + decode, async pair", file_bytes=zt.numel(), out_bytes=2 * half, nlive=info["nlive"],
         nmembers=info["nmembers"], **r)
    r = timed(lambda: D.inflate_parallel_multi(zt))
    assert torch.equal(D.inflate_parallel_multi(zt)[0], want)
    emit(case="a", what="inflate_parallel_multi, end to end", **r)

    def two():
        D.inflate_parallel(zta)
        D.inflate_parallel(ztb)
    r = timed(two)
    assert torch.equal(torch.cat([D.inflate_parallel(zta), D.inflate_parallel(ztb)]), want)
    emit(case="a", what="inflate_parallel on each member alone, summed, end to end", **r)


def bench_b():
    n, page = args.members, 4096
    tb = D.gen_text(n * page, 9).tobytes()
    parts = [gz(tb[k * page:(k + 1) * page]) for k in range(n)]
    lens = np.array([len(p) for p in parts], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1]))
    zt, want = dev(b"".join(parts)), dev(tb)
    fn, out, st, info = multi_pair(zt, n * page)
    r = timed(fn)
    assert int(st[0].item()) & 0xFFFFFFFF == 0 and torch.equal(out, want)
    emit(case="b", what="multi plan + decode, async pair", file_bytes=zt.numel(), out_bytes=n * page, nlive=info["nlive"],
         nmembers=info["nmembers"], nchunks=info["nchunks"], **r)
    r = timed(lambda: D.inflate_parallel_multi(zt))
    emit(case="b", what="inflate_parallel_multi, end to end", **r)
    streams = np.stack([offs, lens], axis=1)
    sizes = np.full(n, page, dtype=np.int64)
    r = timed(lambda: D.inflate_batch(zt, streams, fmt="gzip", sizes=sizes))
    assert torch.equal(D.inflate_batch(zt, streams, fmt="gzip", sizes=sizes)[0][:n * page], want)
    emit(case="b", what="inflate_batch with the true boundaries and sizes (the floor), end to end", **r)
    k = min(1000, n)
    end = int(offs[k - 1] + lens[k - 1])

    def loop():   # what a user can do today: one decode and one synchronisation per member
        pos = 0
        while pos < end:
            _, _, res = D.inflate_batch(zt, [(pos, zt.numel() - pos)], fmt="gzip")
            pos += int(res["in_used"][0])
    r = timed(loop)
    emit(case="b", what=f"host loop of single-member decodes, {k} members", scaled_to_all_ms=round(r["median_ms"] * n / k, 1), **r)


def bench_c():
    n = 2 * args.mb * 1_000_000
    tb = D.gen_text(n, 7).tobytes()
    zt, want = dev(zlib.compress(tb, 6)), dev(tb)
    r = timed(lambda: D.inflate_parallel(zt))
    assert torch.equal(D.inflate_parallel(zt), want)
    emit(case="c", what="inflate_parallel, end to end", tree=args.tree or "this tree", lib=D.LIB_PATH, out_bytes=n, **r)


for c in args.only.split(","):
    {"a": bench_a, "b": bench_b, "c": bench_c}[c]()
