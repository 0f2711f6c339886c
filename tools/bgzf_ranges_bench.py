#!/usr/bin/env python3
"""What reading ranges out of a BGZF file that lies in HBM costs (dmx_bgzf_read_ranges_async), all in
one process on one device, on the project's own BGZF (32 KiB members, the fast parse) of C3's
100 MB and C5's 1 GB of generated text, each resident and indexed once (bgzf_index_gpu).  Batches:

  random   4 096 seeded random ranges of 150..10 000 bytes
  eighth   one range of 1/8 of the file, from its middle
  whole    the whole file as one range

and for each of them, on caller-owned buffers sized by a planning call:

  call          dmx_bgzf_read_ranges_async, CRC check on
  plan_only     the same call with all three capacities 0: the planning launches, no decode, no gather
  members_same  dmx_inflate_members_async with the CRC check on a compact index of the same members,
                built on the host for this comparison: the plain decode of what the batch touches

against the route the parent commit offers for any of them:

  full          dmx_inflate_members_async of the whole file with the CRC check (then slice)

Every figure is the step time of --steps calls back to back on one stream between two
synchronisations after --warmup calls; the best of --repeat runs, all runs listed (their spread is
the run-to-run noise).  Every batch's bytes are compared with the text.  Prints one JSON line and
writes it to --out."""
import argparse
import ctypes
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000000,1000000000")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--nranges", type=int, default=4096)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="", help="file to write the JSON line to (profiles/bgzf_ranges/<label>.json)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    import deflate_compression_amd as D

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

    def figure(fn):
        runs = [timed(fn) for _ in range(args.repeat)]
        return {"ms": round(min(runs), 4), "ms_runs": [round(x, 4) for x in runs]}

    out = {"label": args.label, "steps": args.steps, "warmup": args.warmup, "repeat": args.repeat,
           "device": torch.cuda.get_device_name(0), "files": {}}
    parse = D.DMX_F_LAZY | D.DMX_F_DEEP | D.DMX_F_STORE_CHECK
    for n in [int(x) for x in args.sizes.split(",")]:
        print(f"[{n}] generating and encoding", file=sys.stderr, flush=True)
        d_text = torch.from_numpy(D.gen_text(n, 0xE5818)).cuda()
        enc = D.Encoder(0, n, 32768, 7, D.DMX_BGZF | parse)
        zt, _ = enc.compress_tensor(d_text)
        zt = zt.clone()
        enc.close()
        zn = zt.numel()
        ix, crcs, nblk, total = D.bgzf_index_gpu(zt)
        assert total == n
        res = {"bytes": n, "file_bytes": zn, "nmembers": nblk}
        hidx = ix.cpu().numpy().view(np.uint64).reshape(-1, 3)
        hoff = hidx[:, 1].astype(np.int64)
        hlen = (hidx[:, 2] & 0xFFFFFFFF).astype(np.int64)
        ist = torch.zeros(16, dtype=torch.uint8, device="cuda")

        d_full = torch.empty(n, dtype=torch.uint8, device="cuda")

        def full():
            r = L.dmx_inflate_members_async(vp(zt.data_ptr()), zn, vp(ix.data_ptr()), nblk, vp(d_full.data_ptr()), n,
                                            vp(crcs.data_ptr()), vp(ist.data_ptr()), vp(stream))
            assert r == 0
        res["full"] = dict(figure(full), ok=bool(torch.equal(d_full, d_text)))
        del d_full

        rng = np.random.default_rng(0xB6F)
        lens = rng.integers(150, 10_001, args.nranges)
        batches = {"random": np.stack([rng.integers(0, n - 10_000, args.nranges), lens], axis=1).astype(np.uint64),
                   "eighth": np.array([[n // 2, n // 8]], dtype=np.uint64),
                   "whole": np.array([[0, n]], dtype=np.uint64)}
        for name, rg in batches.items():
            print(f"[{n}] {name}", file=sys.stderr, flush=True)
            k = len(rg)
            rt = torch.from_numpy(rg.view(np.int64).copy()).cuda()
            offs = torch.empty(k + 1, dtype=torch.int64, device="cuda")
            st = torch.empty(32, dtype=torch.uint8, device="cuda")
            w0 = torch.empty(int(L.dmx_bgzf_ranges_work(nblk, k, 0, 0)), dtype=torch.uint8, device="cuda")

            def plan_only():
                r = D.bgzf_read_ranges_async(zt, ix, crcs, nblk, rt, k, 0, None, 0, offs, 0, 0, w0, st, stream)
                assert r == 0
            plan_only()
            need = D.RangesStatus.from_buffer_copy(st.cpu().numpy().tobytes())
            assert need.status == -D.E["E_SZ"]
            mm, sb, ol = need.nmembers, need.scratch_len, need.out_len
            d_out = torch.empty(ol, dtype=torch.uint8, device="cuda")
            work = torch.empty(int(L.dmx_bgzf_ranges_work(nblk, k, mm, sb)), dtype=torch.uint8, device="cuda")

            def call():
                r = D.bgzf_read_ranges_async(zt, ix, crcs, nblk, rt, k, 0, d_out, ol, offs, mm, sb, work, st, stream)
                assert r == 0
            b = {"nranges": k, "nmembers": mm, "scratch_len": sb, "out_len": ol, "work_bytes": work.numel()}
            b["call"] = figure(call)
            rec = D.RangesStatus.from_buffer_copy(st.cpu().numpy().tobytes())
            want = torch.cat([d_text[int(o):int(o) + int(ln)] for o, ln in rg])
            b["call"]["ok"] = rec.status == 0 and bool(torch.equal(d_out, want))
            b["plan_only"] = figure(plan_only)
            # the compact index of the touched members, on the host
            lo = np.searchsorted(hoff, rg[:, 0].astype(np.int64), side="right") - 1
            hi = np.searchsorted(hoff, (rg[:, 0] + rg[:, 1] - 1).astype(np.int64), side="right") - 1
            diff = np.zeros(nblk + 1, dtype=np.int64)
            np.add.at(diff, lo, 1)
            np.add.at(diff, hi + 1, -1)
            needed = np.nonzero(np.cumsum(diff[:nblk]) > 0)[0]
            assert len(needed) == mm and int(hlen[needed].sum()) == sb
            sub = hidx[needed].copy()
            sub[:, 1] = np.concatenate([[0], np.cumsum(hlen[needed])[:-1]]).astype(np.uint64)
            d_sub = torch.from_numpy(sub.view(np.uint8).reshape(-1)).cuda()
            d_subcrc = crcs[torch.from_numpy(needed).cuda()].contiguous()
            d_scr = torch.empty(sb, dtype=torch.uint8, device="cuda")

            def members_same():
                r = L.dmx_inflate_members_async(vp(zt.data_ptr()), zn, vp(d_sub.data_ptr()), mm, vp(d_scr.data_ptr()), sb,
                                                vp(d_subcrc.data_ptr()), vp(ist.data_ptr()), vp(stream))
                assert r == 0
            b["members_same"] = figure(members_same)
            h = ist.cpu().numpy()
            b["members_same"]["ok"] = int(h[:4].view(np.int32)[0]) == 0
            b["call_over_full"] = round(b["call"]["ms"] / res["full"]["ms"], 4)
            b["call_over_members_same"] = round(b["call"]["ms"] / b["members_same"]["ms"], 4)
            b["overhead_ms"] = round(b["call"]["ms"] - b["members_same"]["ms"], 4)
            b["gather_ms_by_difference"] = round(b["call"]["ms"] - b["members_same"]["ms"] - b["plan_only"]["ms"], 4)
            res[name] = b
            del d_out, work, d_sub, d_subcrc, d_scr, want
        out["files"][str(n)] = res
        del d_text, zt, ix, crcs
        torch.cuda.empty_cache()
        if args.out:   # (after every file: a later, larger one may not fit the device)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
