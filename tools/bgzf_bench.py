#!/usr/bin/env python3
"""What the BGZF container costs on C3 (100 MB of generated text, the default fast parse, the
input resident in HBM), beside the gzip container and the zlib stream, all in one process.

Per container two figures: `ms`, the step time of bench.py's timed region (--warmup steps, then
--steps encodes back to back on one stream between two synchronisations; the best of --repeat
runs, all runs listed: their spread is the run-to-run noise), and `stages`, the mean HIP-event
time of every stage and of the whole encode from Encoder.set_timing over --steps encodes (the
event records cost a few microseconds of idle each, so `stages.total` sits above `ms`).  Also
the stand-alone per-block and whole-buffer CRC-32 launches, and the size overhead.

On a tree without the BGZF container (--root DIR, e.g. a checkout of the parent commit with its
library built) only the containers that tree has are reported.  Prints one JSON line."""
import argparse
import ctypes
import gzip
import json
import os
import sys
import time
import zlib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree whose deflate_compression_amd package (and libdmx.so) is measured")
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    import deflate_compression_amd as D

    n = args.bytes
    host = D.gen_text(n, 0xE5818)
    d_in = torch.from_numpy(host).cuda()
    parse = D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK
    kinds = [("zlib", D.DMX_ZLIB)]
    if hasattr(D, "DMX_GZIP"):
        kinds.append(("gzip", D.DMX_GZIP))
    if hasattr(D, "DMX_BGZF"):
        kinds.append(("bgzf", D.DMX_BGZF))
    cap = max(D.max_compressed(n, 32768, f) if f != D.DMX_ZLIB else D.max_compressed(n) for _, f in kinds) + 16
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    enc = D.Encoder(0, n, 32768, 7, D.DMX_ZLIB | parse)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    def encode(flags):
        o = D.Opts(32768, 7, flags | parse, 0)
        return lambda: enc.encode_async(d_in.data_ptr(), n, d_out.data_ptr(), cap, stream, o)

    out = {"label": args.label, "bytes": n, "steps": args.steps, "warmup": args.warmup, "max_chain": 7,
           "flags": "LAZY | DEEP | STORE_CHECK", "device": torch.cuda.get_device_name(0)}
    hb = host.tobytes()
    for name, flags in kinds:
        fn = encode(flags)
        runs = [timed(fn) for _ in range(args.repeat)]
        r = enc.result(stream)
        z = d_out[:int(r.out_len)].cpu().numpy().tobytes()
        rec = {"ms": round(min(runs), 4), "ms_runs": [round(x, 4) for x in runs], "bytes": len(z), "nblocks": int(r.nblocks)}
        rec["ok"] = bool((zlib.decompress(z) if name == "zlib" else gzip.decompress(z)) == hb)
        enc.set_timing(True)
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        st, cnt = enc.stage_times()
        enc.set_timing(False)
        rec["stages"] = {k: round(v, 4) for k, v in st.items()}
        rec["stages_n"] = cnt
        out[name] = rec
    L = D.lib()
    if hasattr(D, "DMX_GZIP"):
        w = torch.zeros(1, dtype=torch.int32, device="cuda")

        def crc():
            L.dmx_crc32_async(enc._ctx, ctypes.c_void_p(d_in.data_ptr()), n, ctypes.c_void_p(w.data_ptr()),
                              ctypes.c_void_p(stream))
        cr = [timed(crc) for _ in range(args.repeat)]
        out["crc32_ms"] = round(min(cr), 4)
        out["crc32_ok"] = bool((int(w.item()) & 0xFFFFFFFF) == zlib.crc32(hb))
    if hasattr(D, "DMX_BGZF"):
        nb = (n + 32767) // 32768
        wb = torch.zeros(nb, dtype=torch.int32, device="cuda")

        def crcb():
            L.dmx_crc32_blocks_async(enc._ctx, ctypes.c_void_p(d_in.data_ptr()), n, 32768, ctypes.c_void_p(wb.data_ptr()),
                                     ctypes.c_void_p(stream))
        cr = [timed(crcb) for _ in range(args.repeat)]
        out["crc32_blocks_ms"] = round(min(cr), 4)
        out["crc32_blocks_GBps"] = round(n / min(cr) / 1e6, 1)
        got = wb.cpu().numpy().view("uint32")
        out["crc32_blocks_ok"] = bool(all(int(got[b]) == zlib.crc32(hb[b * 32768:(b + 1) * 32768]) for b in range(0, nb, 97)))
        out["bgzf_over_gzip"] = round(out["bgzf"]["ms"] / out["gzip"]["ms"], 4)
        out["gzip_over_zlib"] = round(out["gzip"]["ms"] / out["zlib"]["ms"], 4)
        out["bgzf_over_zlib"] = round(out["bgzf"]["ms"] / out["zlib"]["ms"], 4)
        out["bgzf_bytes_over_zlib"] = out["bgzf"]["bytes"] - out["zlib"]["bytes"]
        out["bgzf_framing_bytes"] = 26 * nb + 28
    enc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
