#!/usr/bin/env python3
"""What compressing a batch of independent buffers costs (dmx_encode_batch_async), all in one process
on one device.  Inputs are pieces of C3's generated text, resident in HBM, compressed into zlib
streams with the bench's default options (K = 7, lazy, deep, store check, sw = 32768):

  4k_x65536   65 536 buffers of 4 KiB (one block of 4 KiB each)
  64k_x4096   4 096 buffers of 64 KiB
  1m_x1024    1 024 buffers of 1 MiB
  1m_x64      64 buffers of 1 MiB (a GPU that is not full)

The text is --distinct-mib MiB long (64 by default) and the buffers cycle through it (streams of a
batch may overlap), so the larger batches read every byte several times.  For each input, on
caller-owned buffers and an encoder reserved for the exact block count:

  batch    dmx_encode_batch_async
  concat   (b) one dmx_encode_async over the same bytes laid end to end: where every length is a
           multiple of sw it runs the same blocks, so it is the ceiling the batch should approach,
           less the plan and finish launches

and, on the 64 x 1 MiB set, the parent commit's only route to independent streams:

  loop     (a) a loop of Encoder.compress_tensor per buffer with its result fetch

Every figure is the step time of --steps calls back to back on one stream between two
synchronisations after --warmup calls; the best of --repeat runs, all runs listed.  A sample of
every batch's streams is inflated by zlib and compared with the text, and every stream's check
value with zlib.adler32.  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--loop-steps", type=int, default=3)
    ap.add_argument("--distinct-mib", type=int, default=64)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="", help="file to write the JSON line to (profiles/compress_batch/<label>.json)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    import deflate_compression_amd as D

    L = D.lib()
    SW = 32768
    FLAGS = D.DMX_ZLIB | D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK
    opts = D.Opts(SW, 7, FLAGS, 0)

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
    side = torch.cuda.Stream()   # (a handle of 0 would name the encoder's own stream)
    out = {"label": args.label, "steps": args.steps, "warmup": args.warmup, "repeat": args.repeat,
           "loop_steps": args.loop_steps, "distinct_mib": args.distinct_mib, "device": torch.cuda.get_device_name(0),
           "ncu": torch.cuda.get_device_properties(0).multi_processor_count, "options": "K=7 lazy deep store-check sw=32768",
           "inputs": {}}
    for name, chunk, count in (("4k_x65536", 4096, 65536), ("64k_x4096", 65536, 4096), ("1m_x1024", 1 << 20, 1024),
                               ("1m_x64", 1 << 20, 64)):
        print(f"[{name}]", file=sys.stderr, flush=True)
        total = chunk * count
        offs = (np.arange(count, dtype=np.int64) * chunk) % len(tb)
        desc = np.stack([offs, np.full(count, chunk, np.int64)], axis=1)
        nblk = D.encode_batch_blocks([chunk] * count, SW)
        cap = int(L.dmx_encode_batch_bound(total, count, SW, FLAGS))
        enc = D.Encoder(0, 0, SW, 7, FLAGS)
        enc.reserve_batch(nblk, count, SW, FLAGS)
        with torch.cuda.stream(side):
            dt = torch.from_numpy(desc).cuda()
            d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            res = torch.zeros(count * 4, dtype=torch.int64, device="cuda")
            st = torch.zeros(4, dtype=torch.int64, device="cuda")

            def batch():
                assert D.compress_batch_async(enc, d_text, dt, count, nblk, d_out, cap, res, st, opts) == 0

            b = {"buffers": count, "bytes_each": chunk, "bytes": total, "blocks": nblk}
            b["batch"] = figure(batch, total)
            rec = D.EBatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
            results = res.cpu().numpy().view(np.uint8).reshape(-1).view(D.ERESULT_DTYPE)
            ok = (rec.status, rec.nfailed, rec.nblocks, rec.in_len) == (0, 0, nblk, total)
            adl = {}
            for k in range(count):
                o = int(offs[k])
                if o not in adl:
                    adl[o] = zlib.adler32(tb[o:o + chunk])
                ok = ok and int(results[k]["check"]) == adl[o]
            for k in sorted({0, 1, count // 3, count // 2, count - 2, count - 1}):
                z = d_out[int(results[k]["out_off"]):int(results[k]["out_off"] + results[k]["out_len"])].cpu().numpy().tobytes()
                ok = ok and zlib.decompress(z) == tb[int(offs[k]):int(offs[k]) + chunk]
            b["batch"]["ok"] = bool(ok)
            b["compressed_bytes"] = int(rec.out_len)
            b["ratio"] = round(total / max(1, rec.out_len), 4)
            del d_out
            # (b) one encode over the same bytes end to end
            reps = (total + len(tb) - 1) // len(tb)
            d_cat = d_text.repeat(reps)[:total].contiguous() if total > len(tb) else d_text[:total]
            enc.reserve(total, SW, FLAGS)
            ccap = D.max_compressed(total, SW, FLAGS)
            c_out = torch.empty(ccap, dtype=torch.uint8, device="cuda")
            s = torch.cuda.current_stream().cuda_stream

            def concat():
                enc.encode_async(d_cat.data_ptr(), total, c_out.data_ptr(), ccap, s, opts)

            b["concat"] = figure(concat, total)
            r = enc.result(s)
            b["concat"]["ok"] = r.status == 0 and r.n == total
            b["concat"]["compressed_bytes"] = int(r.out_len)
            b["batch_over_concat"] = round(b["batch"]["ms"] / b["concat"]["ms"], 3)
            del c_out, d_cat
            if name == "1m_x64":
                parts = [d_text[int(o):int(o) + chunk] for o in offs]
                last = []

                def loop():
                    last[:] = [enc.compress_tensor(p, opts=opts) for p in parts]

                b["loop"] = figure(loop, total, steps=args.loop_steps, warmup=1)
                b["loop"]["ok"] = all(r.status == 0 and int(r.out_len) == int(results[k]["out_len"])
                                      for k, (z, r) in enumerate(last))
                b["loop_over_batch"] = round(b["loop"]["ms"] / b["batch"]["ms"], 1)
                del last[:]
        out["inputs"][name] = b
        enc.close()
        del dt, res, st
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
