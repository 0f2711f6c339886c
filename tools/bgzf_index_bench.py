#!/usr/bin/env python3
"""What indexing a BGZF file that already lies in HBM costs on C3 (100 MB of generated text), all in
one process on one device, on the two files of tools/bgzf_read_bench.py -- the project's own BGZF of
the text (32 KiB members, the fast parse) and a foreign one (members of 65 280 input bytes, zlib
level 6, as htslib writes them):

  host_route   what a device-resident file needed before the device index: the file copied to pinned
               host memory, dmx_bgzf_index_max there (one walk, ample capacity), the entries and
               the CRC words copied back
  index        dmx_bgzf_index_async alone (the work buffer sized as bgzf_index_gpu sizes it)
  members      dmx_inflate_members_async alone on the device index, with and without the CRC check
               (the figures of profiles/bgzf_read)
  decode       dmx_bgzf_decode_device end to end, CRC check on

Every figure is the step time of --steps calls back to back on one stream between two
synchronisations after --warmup calls (the host route and the decode synchronise inside every
call); the best of --repeat runs, all runs listed (their spread is the run-to-run noise).  The
device index is compared with the host walk's and everything decoded with the text.  Prints one
JSON line and writes it to --out."""
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
    ap.add_argument("--out", default="", help="file to write the JSON line to (profiles/bgzf_index/<label>.json)")
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

    def figure(runs):
        return {"ms": round(min(runs), 4), "ms_runs": [round(x, 4) for x in runs]}

    hdr = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0])
    parts = []
    for o in range(0, n, args.member):
        blk = hb[o:o + args.member]
        c = zlib.compressobj(args.level, wbits=-15)
        d = c.compress(blk) + c.flush()
        parts.append(hdr + (18 + len(d) + 8 - 1).to_bytes(2, "little") + d + zlib.crc32(blk).to_bytes(4, "little") +
                     len(blk).to_bytes(4, "little"))
    foreign = b"".join(parts) + hdr + bytes([0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    parse = D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK
    enc = D.Encoder(0, n, 32768, 7, D.DMX_BGZF | parse)
    d_text = torch.from_numpy(host).cuda()
    zo, _ = enc.compress_tensor(d_text)
    own = zo.cpu().numpy().tobytes()
    enc.close()

    out = {"label": args.label, "bytes": n, "steps": args.steps, "warmup": args.warmup, "member": args.member,
           "level": args.level, "device": torch.cuda.get_device_name(0), "foreign_bytes": len(foreign), "own_bytes": len(own)}
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    ist = torch.zeros(16, dtype=torch.uint8, device="cuda")

    for name, z in (("own", own), ("foreign", foreign)):
        zn = len(z)
        zt = torch.from_numpy(np.frombuffer(z, np.uint8).copy()).cuda()
        hidx, hcrc, total = D.bgzf_index(z, 65536)
        nb = hcrc.size
        assert total == n
        out[name + "_nmembers"] = nb
        max_cand = zn // 256 + 1024
        wb = int(L.dmx_bgzf_index_work(zn, max_cand))
        out[name + "_work_bytes"] = wb
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        d_idx = torch.empty(max_cand * 24, dtype=torch.uint8, device="cuda")
        d_crc = torch.empty(max_cand, dtype=torch.int32, device="cuda")
        d_st = torch.empty(24, dtype=torch.uint8, device="cuda")

        # (a) the host route: D2H of the file into pinned memory, the walk, H2D of entries and CRC words
        pin_z = torch.empty(zn, dtype=torch.uint8, pin_memory=True)
        pin_idx = torch.empty(max_cand * 24, dtype=torch.uint8, pin_memory=True)
        pin_crc = torch.empty(max_cand, dtype=torch.int32, pin_memory=True)
        cnt, tot = ctypes.c_uint32(0), ctypes.c_uint64(0)

        def host_route():
            pin_z.copy_(zt)   # (synchronous: pinned destination, the call returns when the bytes are there)
            torch.cuda.current_stream().synchronize()
            r = L.dmx_bgzf_index_max(vp(pin_z.data_ptr()), zn, 65536, vp(pin_idx.data_ptr()), vp(pin_crc.data_ptr()), max_cand,
                                     ctypes.byref(cnt), ctypes.byref(tot))
            assert r == 0
            d_idx[:cnt.value * 24].copy_(pin_idx[:cnt.value * 24], non_blocking=True)
            d_crc[:cnt.value].copy_(pin_crc[:cnt.value], non_blocking=True)
            torch.cuda.current_stream().synchronize()

        def index():
            r = L.dmx_bgzf_index_async(vp(zt.data_ptr()), zn, 65536, vp(d_idx.data_ptr()), vp(d_crc.data_ptr()), max_cand,
                                       vp(work.data_ptr()), wb, vp(d_st.data_ptr()), vp(stream))
            assert r == 0

        def members(w):
            def f():
                r = L.dmx_inflate_members_async(vp(zt.data_ptr()), zn, vp(d_idx.data_ptr()), nb, vp(d_out.data_ptr()), n, vp(w),
                                                vp(ist.data_ptr()), vp(stream))
                assert r == 0
            return f
        olen = ctypes.c_uint64(0)

        def decode():
            r = L.dmx_bgzf_decode_device(vp(zt.data_ptr()), zn, vp(d_out.data_ptr()), n, ctypes.byref(olen), 1, vp(stream))
            assert r == 0 and olen.value == n

        def index_ok():
            h = d_st.cpu().numpy()
            rec = (int(h[:4].view(np.int32)[0]), int(h[4:8].view(np.uint32)[0]), int(h[8:16].view(np.uint64)[0]))
            out[name + "_ncand"] = int(h[16:20].view(np.uint32)[0])
            return (rec == (0, nb, n) and d_idx[:nb * 24].cpu().numpy().tobytes() == hidx.tobytes() and
                    d_crc[:nb].cpu().numpy().view(np.uint32).tolist() == hcrc.tolist())

        def text_ok():
            ok = bool(torch.equal(d_out, d_text))
            d_out.zero_()
            return ok

        ra, rb = [], []
        for _ in range(args.repeat):   # alternating
            ra.append(timed(host_route))
            d_idx.zero_()
            rb.append(timed(index))
        out[name + "_host_route"] = dict(figure(ra), ok=cnt.value == nb and tot.value == n)
        out[name + "_index"] = dict(figure(rb), ok=index_ok())
        for key, w in (("members_crc", d_crc.data_ptr()), ("members", 0)):
            runs = [timed(members(w)) for _ in range(args.repeat)]
            h = ist.cpu().numpy()
            out[f"{name}_{key}"] = dict(figure(runs), ok=int(h[:4].view(np.int32)[0]) == 0 and text_ok())
        runs = [timed(decode) for _ in range(args.repeat)]
        out[name + "_decode"] = dict(figure(runs), ok=text_ok())
        out[name + "_index_below_host_route_every_run"] = max(rb) < min(ra)
        out[name + "_index_over_members_crc"] = round(out[name + "_index"]["ms"] / out[name + "_members_crc"]["ms"], 4)
        del zt, work, d_idx, d_crc, pin_z, pin_idx, pin_crc
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
