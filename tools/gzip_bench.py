#!/usr/bin/env python3
"""What the gzip container costs on C3 (100 MB of generated text, the default fast parse, the
input resident in HBM; the loop is bench.py's timed region: --warmup steps, then --steps
encodes back to back on one stream between two synchronisations).

Prints one JSON line: ms per step with DMX_ZLIB; with DMX_GZIP; and the stand-alone
dmx_crc32_async time and GB/s.  On a tree without the gzip container (--root DIR, e.g. a
checkout of the parent commit with its library built) only the zlib figure is reported.
--repeat R times every figure R times: the spread of the zlib figure is the run-to-run noise."""
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
    has_gzip = hasattr(D, "DMX_GZIP")
    parse = D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK
    cap = D.max_compressed(n) + 16
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
    zl = [timed(encode(D.DMX_ZLIB)) for _ in range(args.repeat)]
    r = enc.result(stream)
    out["zlib_ms"] = round(min(zl), 4)
    out["zlib_ms_runs"] = [round(x, 4) for x in zl]
    out["zlib_bytes"] = int(r.out_len)
    if has_gzip:
        gz = [timed(encode(D.DMX_GZIP)) for _ in range(args.repeat)]
        r = enc.result(stream)
        z = d_out[:int(r.out_len)].cpu().numpy().tobytes()
        out["gzip_ms"] = round(min(gz), 4)
        out["gzip_ms_runs"] = [round(x, 4) for x in gz]
        out["gzip_bytes"] = len(z)
        out["gzip_ok"] = bool(gzip.decompress(z) == host.tobytes() and r.adler == zlib.crc32(host))
        w = torch.zeros(1, dtype=torch.int32, device="cuda")
        L = D.lib()

        def crc():
            L.dmx_crc32_async(enc._ctx, ctypes.c_void_p(d_in.data_ptr()), n, ctypes.c_void_p(w.data_ptr()),
                              ctypes.c_void_p(stream))
        cr = [timed(crc) for _ in range(args.repeat)]
        out["crc32_ms"] = round(min(cr), 4)
        out["crc32_ms_runs"] = [round(x, 4) for x in cr]
        out["crc32_GBps"] = round(n / min(cr) / 1e6, 1)
        out["crc32_ok"] = bool((int(w.item()) & 0xFFFFFFFF) == zlib.crc32(host))
        out["gzip_over_zlib"] = round(min(gz) / min(zl), 4)
    enc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
