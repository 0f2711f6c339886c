#!/usr/bin/env python3
"""What reading a BGZF file with 64 KiB members costs on C3 (100 MB of generated text), all in one
process on one device:

  decode    dmx_inflate_members_async on a foreign file -- members of 65 280 input bytes, zlib
            level 6, as htslib writes them -- with and without the per-member CRC check, beside
            dmx_inflate_async on the project's own BGZF of the same text (32 KiB members, the fast
            parse), and dmx_inflate_members_async on that file too.  GB/s of decoded output.
  range CRC dmx_crc32_ranges_async beside dmx_crc32_blocks_async on a uniform 32 768-byte index
            of the text, where both apply.

Every figure is the step time of --steps calls back to back on one stream between two
synchronisations after --warmup calls; the best of --repeat runs, all runs listed (their spread
is the run-to-run noise).  Everything decoded is compared with the text.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--member", type=int, default=65280)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    import deflate_compression_amd as D

    n = args.bytes
    host = D.gen_text(n, 0xE5818)
    hb = host.tobytes()
    L = D.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp = ctypes.c_void_p

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    def rate(runs):
        return {"ms": round(min(runs), 4), "ms_runs": [round(x, 4) for x in runs], "GBps": round(n / min(runs) / 1e6, 2)}

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    # the foreign file: zlib's raw DEFLATE per member behind the 18-byte header
    hdr = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0])
    parts = []
    for o in range(0, n, args.member):
        blk = hb[o:o + args.member]
        c = zlib.compressobj(args.level, wbits=-15)
        d = c.compress(blk) + c.flush()
        parts.append(hdr + (18 + len(d) + 8 - 1).to_bytes(2, "little") + d + zlib.crc32(blk).to_bytes(4, "little") +
                     len(blk).to_bytes(4, "little"))
    foreign = b"".join(parts) + hdr + bytes([0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    # the project's own file: 32 KiB members, the fast parse
    parse = D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK
    enc = D.Encoder(0, n, 32768, 7, D.DMX_BGZF | parse)
    d_text = dev(host)
    zo, _ = enc.compress_tensor(d_text)
    own = zo.cpu().numpy().tobytes()

    out = {"label": args.label, "bytes": n, "steps": args.steps, "warmup": args.warmup, "member": args.member,
           "level": args.level, "device": torch.cuda.get_device_name(0), "foreign_bytes": len(foreign), "own_bytes": len(own)}
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    st = torch.zeros(16, dtype=torch.uint8, device="cuda")

    def status():
        h = st.cpu().numpy()
        return int(h[:4].view(np.int32)[0]), int(h[8:16].view(np.uint64)[0])

    def check():
        ok = status() == (0, n) and bool(torch.equal(d_out, d_text))
        d_out.zero_()
        return ok

    for name, z, bound in (("foreign", foreign, 65536), ("own", own, 32768)):
        idx, crcs, total = D.bgzf_index(z, bound)
        assert total == n
        zt, ix, want = dev(np.frombuffer(z, np.uint8).copy()), dev(idx), dev(crcs.view(np.int32))
        nb = crcs.size
        out[name + "_nmembers"] = nb

        def members(w):
            return lambda: L.dmx_inflate_members_async(vp(zt.data_ptr()), zt.numel(), vp(ix.data_ptr()), nb, vp(d_out.data_ptr()),
                                                       n, vp(w), vp(st.data_ptr()), vp(stream))
        for key, w in (("members_crc", want.data_ptr()), ("members", 0)):
            runs = [timed(members(w)) for _ in range(args.repeat)]
            out[f"{name}_{key}"] = dict(rate(runs), ok=check())
        if bound == 32768:   # the baseline: the 32 KiB reader on the project's own file
            def old():
                L.dmx_inflate_async(vp(zt.data_ptr()), zt.numel(), vp(ix.data_ptr()), nb, vp(d_out.data_ptr()), n,
                                    vp(st.data_ptr()), vp(stream))
            runs = [timed(old) for _ in range(args.repeat)]
            out["own_inflate_async"] = dict(rate(runs), ok=check())

    # the range CRC beside the blocks kernel: a uniform 32 768-byte index of the text
    nb = (n + 32767) // 32768
    rec = np.zeros((nb, 3), np.uint64)
    rec[:, 1] = np.arange(nb, dtype=np.uint64) * 32768
    rec[:, 2] = 32768
    rec[nb - 1, 2] = n - (nb - 1) * 32768
    ix = dev(rec.view(np.uint8).reshape(-1))
    wr = torch.zeros(nb, dtype=torch.int32, device="cuda")
    wb = torch.zeros(nb, dtype=torch.int32, device="cuda")

    def ranges():
        L.dmx_crc32_ranges_async(vp(d_text.data_ptr()), n, vp(ix.data_ptr()), nb, vp(wr.data_ptr()), vp(st.data_ptr()), vp(stream))

    def blocks():
        L.dmx_crc32_blocks_async(enc._ctx, vp(d_text.data_ptr()), n, 32768, vp(wb.data_ptr()), vp(stream))
    st.zero_()
    rr, rb = [], []
    for _ in range(args.repeat):   # alternating
        rr.append(timed(ranges))
        rb.append(timed(blocks))
    got = wr.cpu().numpy().view("uint32")
    out["crc32_ranges"] = dict(rate(rr), ok=bool(torch.equal(wr, wb)) and
                               all(int(got[b]) == zlib.crc32(hb[b * 32768:(b + 1) * 32768]) for b in range(0, nb, 97)))
    out["crc32_blocks"] = rate(rb)
    out["ranges_over_blocks"] = round(min(rr) / min(rb), 3)
    enc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
