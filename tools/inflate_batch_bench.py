#!/usr/bin/env python3
"""What inflating a batch of independent streams costs (dmx_inflate_batch_async), all in one process
on one device.  Inputs are zlib level-6 streams of C3's generated text, resident in HBM and packed
with no padding:

  64k_x4096   4 096 streams of 64 KiB decoded
  1m_x1024    1 024 streams of 1 MiB decoded
  1m_x64      64 streams of 1 MiB decoded (a GPU that is not full)

The text is --distinct-mib MiB long (64 by default) and the streams cycle through it, so the larger
batches hold every compressed stream several times, each copy at its own place in the batch: the
host compresses 64 MiB, not a gigabyte.  For each input, on caller-owned buffers:

  decode    dmx_inflate_batch_async with the decoded lengths given (windows back to back)
  measure   the same call with DMX_BATCH_MEASURE and no output: lengths and statuses only
  two_pass  inflate_batch() without sizes: measure, a device scan, one synchronisation, the
            output's allocation, decode, the copy of the records to the host

against the parent commit's only route for such streams, on the 64 x 1 MiB set:

  stream_loop   a loop of inflate_gpu(z_k, cap) in stream mode (one workgroup of one wave, a
                synchronisation per stream), --loop-steps passes instead of --steps
  zlib_1core    zlib.decompress of the same 64 streams on one core, for scale

Every figure is the step time of --steps calls back to back on one stream between two
synchronisations after --warmup calls; the best of --repeat runs, all runs listed.  Every output is
compared with the text.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time
import zlib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--loop-steps", type=int, default=2)
    ap.add_argument("--distinct-mib", type=int, default=64)
    ap.add_argument("--inputs", default="", help="comma-separated input names (all three by default)")
    ap.add_argument("--lib", default="", help="another libdmx.so to load, e.g. the parent commit's, for A/B runs")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="", help="file to write the JSON line to (profiles/inflate_batch/<label>.json)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    import deflate_compression_amd as D

    if args.lib:   # an older library may lack newer entries: bind only what this tool calls, typed as the tree's
        import ctypes
        other, mine = ctypes.CDLL(os.path.abspath(args.lib)), D.lib()
        for name in ("dmx_inflate_batch_work", "dmx_inflate_batch_async", "dmx_inflate_async", "dmx_gen_text"):
            f, g = getattr(other, name), getattr(mine, name)
            f.argtypes, f.restype = g.argtypes, g.restype
        D._lib = other
    L = D.lib()

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

    text = D.gen_text(args.distinct_mib << 20, 0xE5818)
    d_text = torch.from_numpy(text).cuda()
    tb = text.tobytes()
    out = {"label": args.label, "steps": args.steps, "warmup": args.warmup, "repeat": args.repeat,
           "loop_steps": args.loop_steps, "distinct_mib": args.distinct_mib, "device": torch.cuda.get_device_name(0),
           "ncu": torch.cuda.get_device_properties(0).multi_processor_count, "inputs": {}}
    comp = {}   # (chunk bytes) -> the distinct compressed streams

    def streams_of(chunk):
        if chunk not in comp:
            print(f"compressing {len(tb) // chunk} chunks of {chunk}", file=sys.stderr, flush=True)
            comp[chunk] = [zlib.compress(tb[o:o + chunk], 6) for o in range(0, len(tb), chunk)]
        return comp[chunk]

    only = [s for s in args.inputs.split(",") if s]
    for name, chunk, count in (("64k_x4096", 65536, 4096), ("1m_x1024", 1 << 20, 1024), ("1m_x64", 1 << 20, 64)):
        if only and name not in only:
            continue
        print(f"[{name}]", file=sys.stderr, flush=True)
        zs = streams_of(chunk)
        pick = [zs[k % len(zs)] for k in range(count)]
        lens = np.array([len(z) for z in pick], dtype=np.int64)
        zoff = np.concatenate(([0], np.cumsum(lens)[:-1]))
        zt = torch.frombuffer(bytearray(b"".join(pick)), dtype=torch.uint8).cuda()
        total = chunk * count
        desc = np.stack([zoff, lens, np.arange(count, dtype=np.int64) * chunk, np.full(count, chunk, np.int64)], axis=1)
        dt = torch.from_numpy(desc).cuda()
        res = torch.zeros(count * 4, dtype=torch.int64, device="cuda")
        st = torch.zeros(2, dtype=torch.int64, device="cuda")
        work = torch.empty(int(L.dmx_inflate_batch_work(count)), dtype=torch.uint8, device="cuda")
        d_out = torch.empty(total, dtype=torch.uint8, device="cuda")

        def record():
            return D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())

        def same_as_text(t):
            return all(bool(torch.equal(t[o:o + len(tb)][:min(len(tb), total - o)], d_text[:min(len(tb), total - o)]))
                       for o in range(0, total, len(tb)))

        def decode():
            assert D.inflate_batch_async(zt, dt, count, D.DMX_BATCH_ZLIB, d_out, total, res, work, st) == 0

        def measure():
            assert D.inflate_batch_async(zt, dt, count, D.DMX_BATCH_ZLIB | D.DMX_BATCH_MEASURE, None, 0, res, work, st) == 0

        b = {"streams": count, "decoded_each": chunk, "bytes": total, "compressed_bytes": int(lens.sum()),
             "work_bytes": work.numel()}
        b["decode"] = figure(decode, total)
        rec = record()
        b["decode"]["ok"] = (rec.nfailed, rec.total_out) == (0, total) and same_as_text(d_out)
        b["measure"] = figure(measure, total)
        rec = record()
        b["measure"]["ok"] = (rec.nfailed, rec.total_out) == (0, total)
        sa = desc[:, :2].copy()
        got = []

        def two_pass():
            got[:] = [D.inflate_batch(zt, sa, fmt="zlib")[0]]
        b["two_pass"] = figure(two_pass, total)
        b["two_pass"]["ok"] = same_as_text(got[0])
        del got[:]
        if name == "1m_x64":
            caps = chunk + 16
            parts = [zt[int(o):int(o + n)] for o, n in zip(zoff, lens)]
            last = []

            def stream_loop():
                last[:] = [D.inflate_gpu(p, caps) for p in parts]
            b["stream_loop"] = figure(stream_loop, total, steps=args.loop_steps, warmup=1)
            b["stream_loop"]["ok"] = all(s == 0 and bool(torch.equal(o, d_text[k * chunk:(k + 1) * chunk]))
                                         for k, (o, s) in enumerate(last))
            runs = []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                n = sum(len(zlib.decompress(z)) for z in pick)
                runs.append((time.perf_counter() - t0) * 1e3)
            assert n == total
            b["zlib_1core"] = {"ms": round(min(runs), 2), "ms_runs": [round(x, 2) for x in runs],
                               "GBps": round(total / min(runs) / 1e6, 3)}
            b["decode_over_stream_loop"] = round(b["stream_loop"]["ms"] / b["decode"]["ms"], 1)
        out["inputs"][name] = b
        del zt, d_out, dt, res, work
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
