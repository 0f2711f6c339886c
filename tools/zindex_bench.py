#!/usr/bin/env python3
"""What a seek-point index buys for ONE foreign stream (zindex_build, dmx_inflate_points_async), all
in one process on one device.  Inputs: --mib MiB (100 MB by default) of C3's generated text as one
zlib stream of level 1, 6 and 9 and as the project's own `compress` output, resident in HBM.

For each input and each span (64 KiB, 256 KiB, 1 MiB, 4 MiB):

  npoints, index_bytes   what the index holds (32 + 4 + 32 768 bytes a point)
  build_ms               zindex_build on the host, one core; zlib_1core_ms, zlib.decompress of the same
                         stream on one core, stands beside it for scale
  indexed                the step time of dmx_inflate_points_async over all points on caller-owned
                         buffers with the Adler-32s verified: --steps calls back to back between two
                         synchronisations after --warmup calls, the best of --repeat runs, all listed
  model_ms               the largest point's out_len / 25.3 MB/s: a wave's rate on zlib-6 text, and with
                         npoints <= 1 024 every point has a wave of its own from the start

and at the default span, on every input:

  random_reads           4 096 random ranges of 4 KiB in one zindex_read_ranges call (host planning,
                         the decode of the points touched, the gather, one synchronisation), wall time
  baseline               the parent commit's only route for such a stream: inflate_batch with one
                         stream and sizes= given, one pass (it takes seconds)

Every output is compared with the text.  `acceptance` is the issue's line: at 256 KiB on the level-6
stream the indexed decode is at least npoints / 2 times faster than the baseline.  Prints one JSON
line and writes it to --out."""
import argparse
import json
import os
import sys
import time
import zlib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--mib", type=float, default=100e6 / (1 << 20), help="decoded size (default: 100 MB)")
    ap.add_argument("--inputs", default="", help="comma-separated input names (zlib1, zlib6, zlib9, dmx; all by default)")
    ap.add_argument("--spans", default="65536,262144,1048576,4194304")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="", help="file to write the JSON line to (profiles/zindex/<label>.json)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    import deflate_compression_amd as D

    L = D.lib()
    WAVE_MBPS = 25.3

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def figure(fn, nbytes, steps=None, warmup=None):
        runs = [timed(fn, steps or args.steps, args.warmup if warmup is None else warmup) for _ in range(args.repeat)]
        ms = min(runs)
        return {"ms": round(ms, 4), "ms_runs": [round(x, 4) for x in runs], "GBps": round(nbytes / ms / 1e6, 3)}

    n = int(args.mib * (1 << 20))
    text = D.gen_text(n, 0xE5818)
    d_text = torch.from_numpy(text).cuda()
    tb = text.tobytes()
    spans = [int(s) for s in args.spans.split(",") if s]
    out = {"label": args.label, "steps": args.steps, "warmup": args.warmup, "repeat": args.repeat, "bytes": n,
           "device": torch.cuda.get_device_name(0), "ncu": torch.cuda.get_device_properties(0).multi_processor_count,
           "wave_MBps_model": WAVE_MBPS, "default_span": D.DMX_ZINDEX_DEF_SPAN, "inputs": {}}
    makers = {"zlib1": lambda: zlib.compress(tb, 1), "zlib6": lambda: zlib.compress(tb, 6), "zlib9": lambda: zlib.compress(tb, 9),
              "dmx": lambda: D.compress(tb, max_chain=7, lazy=True)}
    only = [s for s in args.inputs.split(",") if s]
    for name in ("zlib6", "zlib1", "zlib9", "dmx"):
        if only and name not in only:
            continue
        print(f"[{name}] compressing", file=sys.stderr, flush=True)
        z = makers[name]()
        zt = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
        st = torch.zeros(2, dtype=torch.int64, device="cuda")
        runs = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            assert len(zlib.decompress(z)) == n
            runs.append((time.perf_counter() - t0) * 1e3)
        b = {"compressed_bytes": len(z), "zlib_1core_ms": round(min(runs), 1), "zlib_1core_ms_runs": [round(x, 1) for x in runs],
             "spans": {}}
        for span in spans:
            print(f"[{name}] span {span}", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            ix = D.zindex_build(z, span=span)
            build_ms = (time.perf_counter() - t0) * 1e3
            npts = ix.npoints
            pt, at, wt = ix.cuda()
            res = torch.zeros(npts * 4, dtype=torch.int64, device="cuda")
            work = torch.empty(int(L.dmx_inflate_points_work(npts)), dtype=torch.uint8, device="cuda")

            def indexed():
                assert D.inflate_points_async(zt, pt, at, wt, npts, None, None, npts, d_out, n, res, work, st) == 0

            d_out.zero_()
            largest = int(ix.points["out_len"].max())
            s = {"npoints": npts, "index_bytes": ix.nbytes, "index_over_output": round(ix.nbytes / n, 4),
                 "build_ms": round(build_ms, 1), "largest_point": largest, "model_ms": round(largest / WAVE_MBPS / 1e3, 3)}
            s["indexed"] = figure(indexed, n)
            rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
            s["indexed"]["ok"] = (rec.nfailed, rec.total_out) == (0, n) and bool(torch.equal(d_out, d_text))
            s["indexed_over_model"] = round(s["indexed"]["ms"] / s["model_ms"], 3)
            if span == D.DMX_ZINDEX_DEF_SPAN:
                rng = np.random.default_rng(17)
                ranges = np.stack([rng.integers(0, n - 4096, 4096), np.full(4096, 4096)], axis=1).astype(np.int64)
                got = []
                rr = []
                for _ in range(args.repeat):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got[:] = D.zindex_read_ranges(zt, ix, ranges)
                    torch.cuda.synchronize()
                    rr.append((time.perf_counter() - t0) * 1e3)
                flat = got[0].cpu().numpy()
                ok = all(flat[q * 4096:(q + 1) * 4096].tobytes() == tb[int(o):int(o) + 4096] for q, o in enumerate(ranges[:, 0]))
                touched = len(set(int(k) for o in ranges[:, 0] for k in
                                  (np.searchsorted(ix.points["out_off"], [o, o + 4095], side="right") - 1)))
                s["random_reads"] = {"ranges": 4096, "each": 4096, "points_touched_at_least": touched, "ms": round(min(rr), 3),
                                     "ms_runs": [round(x, 3) for x in rr], "ok": ok,
                                     "over_whole_decode": round(min(rr) / s["indexed"]["ms"], 3)}
                del got[:]
                t0 = time.perf_counter()
                one = D.zindex_pread(zt, ix, n // 2 + 123, 4096)
                torch.cuda.synchronize()
                s["one_pread_4k_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                assert one.cpu().numpy().tobytes() == tb[n // 2 + 123:n // 2 + 123 + 4096]
            b["spans"][str(span)] = s
            del pt, at, wt, res, work, ix
        if not args.no_baseline:
            print(f"[{name}] baseline", file=sys.stderr, flush=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o, _, results = D.inflate_batch(zt, np.array([[0, len(z)]], dtype=np.int64), fmt="zlib", sizes=[n])
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            b["baseline"] = {"ms": round(ms, 1), "passes": 1, "MBps": round(n / ms / 1e3, 2),
                             "ok": int(results["status"][0]) == 0 and bool(torch.equal(o, d_text))}
            del o
            for span, s in b["spans"].items():
                s["baseline_over_indexed"] = round(b["baseline"]["ms"] / s["indexed"]["ms"], 1)
        out["inputs"][name] = b
        del zt, d_out
    z6 = out["inputs"].get("zlib6", {})
    s = z6.get("spans", {}).get(str(D.DMX_ZINDEX_DEF_SPAN))
    if s and "baseline" in z6:
        out["acceptance"] = {"span": D.DMX_ZINDEX_DEF_SPAN, "npoints": s["npoints"], "baseline_ms": z6["baseline"]["ms"],
                             "indexed_ms": s["indexed"]["ms"], "ratio": s["baseline_over_indexed"],
                             "needed": s["npoints"] / 2, "ok": s["baseline_over_indexed"] >= s["npoints"] / 2}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
