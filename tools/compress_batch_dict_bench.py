#!/usr/bin/env python3
"""What compressing a batch of independent buffers against a preset dictionary costs
(dmx_encode_batch_dict_async), all in one process on one device.  Inputs are pieces of C3's generated
text, resident in HBM, compressed into zlib streams with FDICT at K = 7 lazy, sw = 32768, against one
shared dictionary of 32 KiB (the first 32 KiB of the same generator with another seed):

  4k_x65536   65 536 pages of 4 KiB (one block each: every block sees the dictionary)
  64k_x4096   4 096 buffers of 64 KiB (two blocks each: only the first sees the dictionary)

For each input, on caller-owned buffers and an encoder reserved for the exact block count:

  dict      dmx_encode_batch_dict_async, the resident form of the history search (the default)
  simple    the same with DMX_HOOK_BDICT_SIMPLE (a workgroup per table entry); on the 4 KiB shape the two
            forms run alternating, --repeat runs each
  plain     dmx_encode_batch_async on the same buffers (no dictionary): the size and time to compare with
  stages    the context's stage times of the dict form, in a run of its own (event records between the
            kernels cost a few us each): [plan + chains + history + K0, K1, K2, K3, K4 + finish]

and a host loop of single dmx_encode_async dictionary encodes with their result fetch over --loop-pages of
the same pages.  Every figure is the step time of --steps calls back to back on one stream between two
synchronisations after --warmup calls; all runs are listed.  Every stream of the dict form is decoded by
zlib.decompressobj(zdict=) and compared with its page, its check value with zlib.adler32, and the
simple form's output with the resident form's, byte for byte.  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--loop-pages", type=int, default=1024)
    ap.add_argument("--distinct-mib", type=int, default=64)
    ap.add_argument("--scale", type=int, default=1, help="divide the buffer counts by this (rehearsals)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="", help="file to write the JSON line to (profiles/compress_batch_dict/<label>.json)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    import deflate_compression_amd as D

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    L = D.lib()
    SW = 32768
    PARSE = D.DMX_F_LAZY
    FLAGS = D.DMX_ZLIB | D.DMX_F_DICT | D.DMX_F_FDICT | PARSE
    opts = D.Opts(SW, 7, FLAGS, 0)
    popts = D.Opts(SW, 7, D.DMX_ZLIB | PARSE, 0)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def summary(runs, nbytes):
        ms = min(runs)
        return {"ms": round(ms, 4), "ms_runs": [round(x, 4) for x in runs], "GBps": round(nbytes / ms / 1e6, 3)}

    text = D.gen_text(args.distinct_mib << 20, 0xE5818)
    zd = D.gen_text(SW, 0xD1C7).tobytes()
    d_text = torch.from_numpy(text).cuda()
    d_dict = torch.frombuffer(bytearray(zd), dtype=torch.uint8).cuda()
    ddesc = torch.tensor([[0, SW]], dtype=torch.int64, device="cuda")
    tb = text.tobytes()
    side = torch.cuda.Stream()   # (a handle of 0 would name the encoder's own stream)
    out = {"label": args.label, "steps": args.steps, "warmup": args.warmup, "repeat": args.repeat,
           "loop_pages": args.loop_pages, "distinct_mib": args.distinct_mib, "device": torch.cuda.get_device_name(0),
           "ncu": torch.cuda.get_device_properties(0).multi_processor_count,
           "options": "K=7 lazy sw=32768 zlib FDICT, one shared dictionary of 32 KiB", "inputs": {}}
    for name, chunk, count in (("4k_x65536", 4096, 65536 // args.scale), ("64k_x4096", 65536, 4096 // args.scale)):
        print(f"[{name}]", file=sys.stderr, flush=True)
        total = chunk * count
        offs = (np.arange(count, dtype=np.int64) * chunk) % len(tb)
        desc = np.stack([offs, np.full(count, chunk, np.int64)], axis=1)
        nblk = D.encode_batch_blocks([chunk] * count, SW)
        cap = int(L.dmx_encode_batch_dict_bound(total, count, SW, FLAGS))
        enc = D.Encoder(0, 0, SW, 7, D.DMX_ZLIB | PARSE)
        enc.reserve_batch_dict(nblk, count, 1, SW, FLAGS)
        with torch.cuda.stream(side):
            dt = torch.from_numpy(desc).cuda()
            d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            res = torch.zeros(count * 4, dtype=torch.int64, device="cuda")
            st = torch.zeros(4, dtype=torch.int64, device="cuda")

            def batch():
                assert D.compress_batch_dict_async(enc, d_text, dt, count, nblk, d_dict, ddesc, 1, None, d_out, cap, res, st,
                                                   opts) == 0

            def plain():
                assert D.compress_batch_async(enc, d_text, dt, count, nblk, d_out, cap, res, st, popts) == 0

            b = {"buffers": count, "bytes_each": chunk, "bytes": total, "blocks": nblk}
            # the two forms alternating: resident, simple, resident, simple, ...
            runs = {"dict": [], "simple": []}
            outputs = {}
            for _ in range(args.repeat):
                for form, hook in (("dict", 0), ("simple", 1)):
                    enc.set_hook("bdict_simple", hook)
                    runs[form].append(timed(batch, args.steps, args.warmup))
                    if form not in outputs:
                        rec = D.EBatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
                        outputs[form] = (d_out[:rec.out_len].cpu().numpy().tobytes(), res.cpu().numpy().tobytes(), rec)
            enc.set_hook("bdict_simple", 0)
            b["dict"] = summary(runs["dict"], total)
            b["simple"] = summary(runs["simple"], total)
            b["resident_wins_every_run"] = bool(max(runs["dict"]) < min(runs["simple"]))
            b["simple"]["same_bytes"] = outputs["dict"][:2] == outputs["simple"][:2]
            zbytes, rbytes, rec = outputs["dict"]
            results = np.frombuffer(rbytes, dtype=np.uint8).view(D.ERESULT_DTYPE)
            ok = (rec.status, rec.nfailed, rec.nblocks, rec.in_len) == (0, 0, nblk, total)
            seen = {}
            for k in range(count):   # every output decoded and compared (the buffers cycle: once per distinct one)
                o = int(offs[k])
                z = zbytes[int(results[k]["out_off"]):int(results[k]["out_off"] + results[k]["out_len"])]
                if o in seen:
                    ok = ok and z == seen[o]
                    continue
                seen[o] = z
                dz = zlib.decompressobj(zdict=zd)
                ok = ok and dz.decompress(z) == tb[o:o + chunk] and dz.eof
                ok = ok and int(results[k]["check"]) == zlib.adler32(tb[o:o + chunk])
            b["dict"]["ok"] = bool(ok)
            b["compressed_bytes"] = int(rec.out_len)
            b["ratio"] = round(total / max(1, rec.out_len), 4)
            # the old entry on the same buffers
            enc.reserve_batch(nblk, count, SW, popts.flags)
            b["plain"] = summary([timed(plain, args.steps, args.warmup) for _ in range(args.repeat)], total)
            prec = D.EBatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
            b["plain"]["ok"] = (prec.status, prec.nfailed) == (0, 0)
            b["plain"]["compressed_bytes"] = int(prec.out_len)
            b["dict_over_plain_bytes"] = round(rec.out_len / max(1, prec.out_len), 4)
            b["dict_over_plain_ms"] = round(b["dict"]["ms"] / b["plain"]["ms"], 3)
            # the stage times, in a run of their own
            enc.set_timing(True)
            timed(batch, args.steps, args.warmup)
            tm, cnt = enc.stage_times()   # ("pre": the plan, the DICTIDs, the chains, the history search and K0)
            b["stages_ms"] = {k: round(v, 4) for k, v in tm.items()}
            b["stages_ms"]["encodes"] = cnt
            enc.set_timing(False)
            if name == "4k_x65536":   # the route a caller had before: a loop of single dictionary encodes
                npg = min(args.loop_pages, count)
                parts = [d_text[int(o):int(o) + chunk] for o in offs[:npg]]
                lo = D.Opts(SW, 7, FLAGS, 0)
                lo.dict, lo.dict_len = d_dict.data_ptr(), SW
                last = []

                def loop():
                    last[:] = [enc.compress_tensor(p, opts=lo) for p in parts]

                b["loop"] = summary([timed(loop, 1, 1) for _ in range(args.repeat)], npg * chunk)
                b["loop"]["pages"] = npg
                b["loop"]["ok"] = all(r.status == 0 and z.cpu().numpy().tobytes() ==
                                      zbytes[int(results[k]["out_off"]):int(results[k]["out_off"] + results[k]["out_len"])]
                                      for k, (z, r) in enumerate(last))
                b["loop_over_batch_per_page"] = round((b["loop"]["ms"] / npg) / (b["dict"]["ms"] / count), 1)
                del last[:]
            del d_out
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
