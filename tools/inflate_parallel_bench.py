#!/usr/bin/env python3
"""The numbers of profiles/inflate_parallel/README.md, "The rebuilt decode": one foreign stream of
100 MB resident in HBM, decoded in one pass (inflate_parallel: the device plan and the decode), beside
the two routes the library had before -- inflate_batch with that one stream and its length given, and
zindex_build + inflate_indexed as a first read -- in the same process, alternating.

Method, as the old table's: one warm-up, then `--calls` calls back to back between two
synchronisations, the best of `--runs` runs and their spread; every output is compared with the
input.  plan / decode / both are the async pair on buffers allocated once; e2e is inflate_parallel
itself, with its synchronisation and its allocations.  The serial routes are one call a run (they
take seconds).  One JSON line per row, then the table in Markdown.

    python tools/inflate_parallel_bench.py                  # every row
    python tools/inflate_parallel_bench.py --rows z6 --cuts 16,64 --no-serial
    rocprofv3 --kernel-trace --stats -d out -- python tools/inflate_parallel_bench.py --rows z6 --cuts 16 --profile
"""
import argparse
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import deflate_compression_amd as D


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


def bench_row(name, z, data_t, cut, calls, runs, serial, profile):
    L = D.lib()
    zt = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    n = data_t.numel()
    row = {"row": name, "cut": cut, "stream_bytes": len(z), "out_bytes": n}
    info = {}
    out = D.inflate_parallel(zt, chunk_bytes=cut, info=info)
    assert torch.equal(out, data_t), name
    row.update({k: info[k] for k in ("route", "nchunks", "ncand", "nlive", "ndead", "status", "gave_up")})
    if profile:   # one more plan + decode for the kernel trace, nothing else
        D.inflate_parallel(zt, chunk_bytes=cut)
        sync()
        return row
    e2e = runs_of(lambda: D.inflate_parallel(zt, chunk_bytes=cut), calls, runs)
    row["e2e_ms"] = ms(e2e)
    if info["route"] == "parallel":
        plan = torch.empty(L.dmx_inflate_parallel_plan_work(zt.numel(), cut), dtype=torch.uint8, device="cuda")
        work = torch.empty(info["work_len"], dtype=torch.uint8, device="cuda")
        dst = torch.empty(n, dtype=torch.uint8, device="cuda")
        st = torch.empty(7, dtype=torch.int64, device="cuda")

        def plan_call():
            assert D.inflate_parallel_plan_async(zt, 0, cut, plan) == 0

        def decode_call():
            assert D.inflate_parallel_decode_async(zt, plan, info["nlive"], dst, n, work, True, st) == 0

        def both():
            plan_call()
            decode_call()

        row["plan_ms"] = ms(runs_of(plan_call, calls, runs))
        row["decode_ms"] = ms(runs_of(decode_call, calls, runs))
        row["both_ms"] = ms(runs_of(both, calls, runs))
        assert D.ParStatus.from_buffer_copy(st.cpu().numpy().tobytes()).status == 0 and torch.equal(dst, data_t)
        row["gbps"] = round(n / min(row["both_ms"]) / 1e6, 2)
    if serial:
        def batch_call():
            o, _, _ = D.inflate_batch(zt, [(0, zt.numel())], sizes=[n])
            return o

        def zindex_call():
            return D.inflate_indexed(zt, D.zindex_build(z))

        assert torch.equal(batch_call(), data_t) and torch.equal(zindex_call(), data_t)
        b, x = [], []
        for _ in range(runs):   # alternating, one call a run
            b += runs_of(batch_call, 1, 1)
            x += runs_of(zindex_call, 1, 1)
        row["batch_ms"], row["zindex_first_read_ms"] = ms(b), ms(x)
        row["ahead_in_every_run"] = bool(max(row["e2e_ms"]) < min(min(b), min(x)) * 1e3)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mb", type=int, default=100)
    ap.add_argument("--rows", default="z6,z1,z9,own,noise", help="z1, z6, z9, own (the project's encode), noise")
    ap.add_argument("--cuts", default="16,32,64,128", help="KiB, for the z6 row; the other rows use --cut")
    ap.add_argument("--cut", type=int, default=64)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-serial", action="store_true", help="leave the two serial routes out")
    ap.add_argument("--profile", action="store_true", help="one plan + decode a row and nothing else (under rocprofv3)")
    a = ap.parse_args()
    n = a.mb * 1_000_000
    text = D.gen_text(n, 0xE5818)   # bench.py's C3 text
    text_t = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    rows = []
    for r in a.rows.split(","):
        if r in ("z1", "z6", "z9"):
            z = zlib.compress(text.tobytes(), int(r[1]))
            cuts = [int(c) for c in a.cuts.split(",")] if r == "z6" else [a.cut]
            for c in cuts:
                rows.append(bench_row(f"text, zlib {r[1]}", z, text_t, c << 10, a.calls, a.runs,
                                      not a.no_serial and (r != "z6" or c == cuts[0]), a.profile))
                print(json.dumps(rows[-1]), flush=True)
        elif r == "own":
            z = D.compress(text.tobytes())
            rows.append(bench_row("text, own encode", z, text_t, a.cut << 10, a.calls, a.runs, not a.no_serial, a.profile))
            print(json.dumps(rows[-1]), flush=True)
        elif r == "noise":
            noise = D.gen_random(n)
            z = zlib.compress(noise.tobytes(), 6)
            rows.append(bench_row("noise (stored blocks)", z, torch.from_numpy(np.ascontiguousarray(noise)).cuda(), a.cut << 10,
                                  a.calls, a.runs, not a.no_serial, a.profile))
            print(json.dumps(rows[-1]), flush=True)
        else:
            raise SystemExit("unknown row " + r)
    if a.profile:
        return
    f = lambda v: f"{min(v):.1f} (+{max(v) - min(v):.1f})" if v else ""
    print("| input | cut | route | chunks / candidates / live / dead | plan ms | decode ms | plan + decode | GB/s | "
          "`inflate_parallel` | `inflate_batch`, one stream | `zindex_build` + `inflate_indexed` |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['row']} | {r['cut'] >> 10} KiB | {r['route']} | {r['nchunks']} / {r['ncand']} / {r['nlive']} / {r['ndead']} | "
              f"{f(r.get('plan_ms'))} | {f(r.get('decode_ms'))} | {f(r.get('both_ms'))} | {r.get('gbps', '')} | {f(r['e2e_ms'])} | "
              f"{f(r.get('batch_ms'))} | {f(r.get('zindex_first_read_ms'))} |")


if __name__ == "__main__":
    main()
