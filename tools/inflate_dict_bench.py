#!/usr/bin/env python3
"""What a preset dictionary costs and buys on small streams (dmx_inflate_batch_dict_async): 65 536
zlib level-6 streams of 4 KiB pages of C3's generated text, resident in HBM and packed with no
padding, decoded twice on caller-owned buffers with the decoded lengths given:

  plain    written without a dictionary, decoded by dmx_inflate_batch_async
  dict     written against one shared 32 KiB dictionary (text of the same generator, another seed;
           zlib's zdict=, so every stream has FDICT), decoded by dmx_inflate_batch_dict_async

--distinct pages are compressed on the host (4 096 by default) and the streams cycle through them.
Every figure is the step time of --steps calls back to back on one stream between two
synchronisations after --warmup calls; the best of --repeat runs, all runs listed.  Every output is
compared with the pages.  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--page", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=4096)
    ap.add_argument("--dict-bytes", type=int, default=32768)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    import deflate_compression_amd as D

    L = D.lib()
    n, page = args.streams, args.page
    text = D.gen_text(args.distinct * page, 0xE5818).tobytes()
    zd = D.gen_text(args.dict_bytes, 0xD1C7).tobytes()
    pages = [text[o:o + page] for o in range(0, len(text), page)]
    want = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    total = n * page

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    out = {"streams": n, "page": page, "distinct": args.distinct, "dict_bytes": len(zd), "bytes": total,
           "steps": args.steps, "warmup": args.warmup, "repeat": args.repeat, "device": torch.cuda.get_device_name(0)}
    dbuf = torch.frombuffer(bytearray(zd), dtype=torch.uint8).cuda()
    dicts_t = torch.tensor([[0, len(zd)]], dtype=torch.int64, device="cuda")
    for name in ("plain", "dict"):
        zs = []
        for p in pages:
            c = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=zd) if name == "dict" else zlib.compressobj(6)
            zs.append(c.compress(p) + c.flush())
        pick = [zs[k % len(zs)] for k in range(n)]
        lens = np.array([len(z) for z in pick], dtype=np.int64)
        zoff = np.concatenate(([0], np.cumsum(lens)[:-1]))
        zt = torch.frombuffer(bytearray(b"".join(pick)), dtype=torch.uint8).cuda()
        desc = np.stack([zoff, lens, np.arange(n, dtype=np.int64) * page, np.full(n, page, np.int64)], axis=1)
        dt = torch.from_numpy(desc).cuda()
        res = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
        st = torch.zeros(2, dtype=torch.int64, device="cuda")
        d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
        if name == "dict":
            work = torch.empty(int(L.dmx_inflate_batch_dict_work(n, 1)), dtype=torch.uint8, device="cuda")

            def call():
                assert D.inflate_batch_dict_async(zt, dt, n, D.DMX_BATCH_ZLIB, dbuf, dicts_t, 1, None, d_out, total, res, work, st) == 0
        else:
            work = torch.empty(int(L.dmx_inflate_batch_work(n)), dtype=torch.uint8, device="cuda")

            def call():
                assert D.inflate_batch_async(zt, dt, n, D.DMX_BATCH_ZLIB, d_out, total, res, work, st) == 0
        runs = [timed(call) for _ in range(args.repeat)]
        rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
        ok = (rec.nfailed, rec.total_out) == (0, total) and all(
            bool(torch.equal(d_out[o:o + len(text)], want[:min(len(text), total - o)])) for o in range(0, total, len(text)))
        ms = min(runs)
        out[name] = {"ms": round(ms, 4), "ms_runs": [round(x, 4) for x in runs], "GBps": round(total / ms / 1e6, 3),
                     "compressed_bytes": int(lens.sum()), "ratio": round(total / int(lens.sum()), 3), "ok": ok}
        del zt, d_out, dt, res, work
    out["dict_over_plain_ms"] = round(out["dict"]["ms"] / out["plain"]["ms"], 4)
    out["dict_over_plain_size"] = round(out["dict"]["compressed_bytes"] / out["plain"]["compressed_bytes"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
