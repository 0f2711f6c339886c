#!/usr/bin/env python3
"""What opening and reading a ZIP archive that lies in HBM costs, all in one process on one device:

  index     zip_index_gpu's device call (dmx_zip_index_async on caller-owned buffers) on archives of
            --entries small stored entries, against the only route there was before: the archive
            copied to the host and zipfile.ZipFile(...).infolist() there
  deflated  dmx_zip_read_async (CRC-32 check on) on 4 096 entries of 64 KiB and 1 024 of 1 MiB of
            generated text (16 distinct texts, every entry its own copy of one of them), against the
            same decode kernel told every boundary: dmx_inflate_batch_async on the same streams
            wrapped as gzip members, which is the batch decode plus the same CRC-32 pass; and both
            without the check (raw streams / verify off)
  stored    the copy kernel on 64 stored entries of 16 MiB (verify off) against torch's
            device-to-device copy of the same bytes

Every figure is the step time of --steps calls back to back on one stream between two
synchronisations after --warmup calls; all --repeat runs are listed (their spread is the run-to-run
noise), the best is `ms`.  Everything decoded is compared with the input.  Prints one JSON line per
section and writes them to --out/<section>.json."""
import argparse
import io
import json
import os
import struct
import sys
import time
import zipfile
import zlib


def make_zip(entries) -> bytes:
    """entries: (name bytes, method, payload, crc, usize)"""
    body, central = [], []
    off = 0
    for name, method, comp, crc, usize in entries:
        lh = struct.pack("<IHHHHHIIIHH", 0x04034B50, 20, 0, method, 0, 0x21, crc, len(comp), usize, len(name), 0) + name
        body.append(lh)
        body.append(comp)
        central.append(struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 20, 20, 0, method, 0, 0x21, crc, len(comp), usize,
                                   len(name), 0, 0, 0, 0, 0, off) + name)
        off += len(lh) + len(comp)
    cd = b"".join(central)
    n = len(entries)
    if n >= 0xFFFF:
        tail = struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, n, n, len(cd), off)
        tail += struct.pack("<IIQI", 0x07064B50, 0, off + len(cd), 1)
        tail += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, 0xFFFF, 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0)
    else:
        tail = struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, n, n, len(cd), off, 0)
    return b"".join(body) + cd + tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="1024,65536,1000000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sections", default="index,deflated,stored")
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks every size (a rehearsal)")
    ap.add_argument("--out", default="profiles/zip")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    import deflate_compression_amd as D

    assert torch.cuda.is_available(), "zip_bench needs a GPU"
    L = D.lib()
    dev = torch.cuda.get_device_name(0)

    def timed(fn, steps=args.steps, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def figure(runs):
        return {"ms": round(min(runs), 4), "ms_runs": [round(x, 4) for x in runs], "spread_ms": round(max(runs) - min(runs), 4)}

    def emit(name, rec):
        rec = dict(rec, section=name, device=dev, steps=args.steps, warmup=args.warmup, repeat=args.repeat, scale=args.scale)
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            f.write(line + "\n")

    def upload(z):
        return torch.from_numpy(np.frombuffer(z, np.uint8).copy()).cuda()

    sections = args.sections.split(",")
    if "index" in sections:
        rec = {}
        for n in [max(1, int(int(x) * args.scale)) for x in args.entries.split(",")]:
            z = make_zip([(b"entry/%07d" % i, 0, b"%08d" % i, zlib.crc32(b"%08d" % i), 8) for i in range(n)])
            zt = upload(z)
            cap = n
            work = torch.empty(int(L.dmx_zip_index_work(len(z), cap + 1024)), dtype=torch.uint8, device="cuda")
            ent = torch.empty(cap * 64, dtype=torch.uint8, device="cuda")
            st = torch.empty(40, dtype=torch.uint8, device="cuda")

            def index():
                assert D.zip_index_async(zt, ent, cap, work, st) == 0

            infos = []

            def host_route():
                b = zt.cpu().numpy().tobytes()
                with zipfile.ZipFile(io.BytesIO(b)) as zf:
                    infos[:] = [len(zf.infolist())]

            slow = n > 100000   # zipfile takes seconds there: one call per run
            ra = [timed(index) for _ in range(args.repeat)]
            rb = [timed(host_route, 1 if slow else 3, 0 if slow else 1) for _ in range(2 if slow else args.repeat)]
            s = D.ZipStatus.from_buffer_copy(st.cpu().numpy().tobytes())
            ref = D.zip_index(z)
            ok = (s.status, s.nentries) == (0, n) and ent.cpu().numpy().tobytes() == ref.host.tobytes() and infos == [n]
            rec[f"n{n}"] = {"zbytes": len(z), "work_bytes": work.numel(), "index": figure(ra), "host_route": figure(rb), "ok": ok,
                            "host_over_index": round(min(rb) / min(ra), 2)}
            del zt, work, ent
        emit("index", rec)

    if "deflated" in sections:
        rec = {}
        for count, size in ((4096, 64 << 10), (1024, 1 << 20)):
            count = max(16, int(count * args.scale))
            texts = [D.gen_text(size, 100 + k).tobytes() for k in range(16)]
            comps = []
            for t in texts:
                c = zlib.compressobj(6, zlib.DEFLATED, -15)
                comps.append(c.compress(t) + c.flush())
            crcs = [zlib.crc32(t) for t in texts]
            z = make_zip([(b"t/%05d" % i, 8, comps[i % 16], crcs[i % 16], size) for i in range(count)])
            zt = upload(z)
            ix = D.zip_index_gpu(zt)
            total = ix.out_len
            assert total == count * size
            # the yardstick's inputs: the same streams as raw streams and as gzip members
            gz = b"".join(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + comps[i % 16] +
                          struct.pack("<II", crcs[i % 16], size) for i in range(count))
            gt = upload(gz)
            desc_raw = np.zeros((count, 4), dtype=np.int64)
            desc_raw[:, 0], desc_raw[:, 1] = ix.host["data_off"], ix.host["csize"]
            desc_raw[:, 2], desc_raw[:, 3] = ix.host["out_off"], size
            desc_gz = desc_raw.copy()
            glen = np.array([18 + len(comps[i % 16]) for i in range(count)], dtype=np.int64)
            desc_gz[:, 0], desc_gz[:, 1] = np.concatenate(([0], np.cumsum(glen)[:-1])), glen
            d_raw, d_gz = torch.from_numpy(desc_raw).cuda(), torch.from_numpy(desc_gz).cuda()
            out = torch.empty(total, dtype=torch.uint8, device="cuda")
            offsets = torch.empty(count + 1, dtype=torch.int64, device="cuda")
            res = torch.zeros(count * 4, dtype=torch.int64, device="cuda")
            st = torch.empty(2, dtype=torch.int64, device="cuda")
            bwork = torch.empty(int(L.dmx_inflate_batch_work(count)), dtype=torch.uint8, device="cuda")
            zwork = torch.empty(int(L.dmx_zip_read_work(count)), dtype=torch.uint8, device="cuda")
            want = torch.from_numpy(np.frombuffer(b"".join(texts), np.uint8).copy()).cuda()

            def check():
                r = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
                good = (r.nfailed, r.total_out) == (0, total)
                v = out.view(count, size)
                for k in range(16):
                    good = good and bool((v[k::16] == want[k * size:(k + 1) * size]).all())
                out.zero_()
                return good

            def yard_gzip():
                assert D.inflate_batch_async(gt, d_gz, count, D.DMX_BATCH_GZIP, out, total, res, bwork, st) == 0

            def yard_raw():
                assert D.inflate_batch_async(zt, d_raw, count, D.DMX_BATCH_RAW, out, total, res, bwork, st) == 0

            def zip_verify():
                assert D.zip_read_async(zt, ix.entries, count, None, count, D.DMX_ZIP_VERIFY, out, total, offsets, res, zwork, st) == 0

            def zip_plain():
                assert D.zip_read_async(zt, ix.entries, count, None, count, 0, out, total, offsets, res, zwork, st) == 0

            runs = {k: [] for k in ("yard_gzip", "zip_verify", "yard_raw", "zip_plain")}
            oks = {}
            for _ in range(args.repeat):   # alternating
                for k, fn in (("yard_gzip", yard_gzip), ("zip_verify", zip_verify), ("yard_raw", yard_raw), ("zip_plain", zip_plain)):
                    runs[k].append(timed(fn))
                    oks[k] = oks.get(k, True) and check()
            r = {k: dict(figure(v), ok=oks[k], gb_s=round(total / min(v) / 1e6, 2)) for k, v in runs.items()}
            r["zbytes"], r["out_bytes"] = len(z), total
            r["verify_inside_yardstick_spread"] = abs(r["zip_verify"]["ms"] - r["yard_gzip"]["ms"]) <= r["yard_gzip"]["spread_ms"]
            r["plain_inside_yardstick_spread"] = abs(r["zip_plain"]["ms"] - r["yard_raw"]["ms"]) <= r["yard_raw"]["spread_ms"]
            rec[f"{count}x{size}"] = r
            del zt, gt, out, want
        emit("deflated", rec)

    if "stored" in sections:
        count, size = 64, max(1 << 16, int((16 << 20) * args.scale))
        blob = D.gen_random(size, 77).tobytes()
        crc = zlib.crc32(blob)
        z = make_zip([(b"s/%03d" % i, 0, blob, crc, size) for i in range(count)])
        zt = upload(z)
        ix = D.zip_index_gpu(zt)
        total = count * size
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        offsets = torch.empty(count + 1, dtype=torch.int64, device="cuda")
        res = torch.zeros(count * 4, dtype=torch.int64, device="cuda")
        st = torch.empty(2, dtype=torch.int64, device="cuda")
        zwork = torch.empty(int(L.dmx_zip_read_work(count)), dtype=torch.uint8, device="cuda")
        src = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda().repeat(count)
        want = src[:size].clone()

        def check():
            good = bool((out.view(count, size) == want).all())
            out.zero_()
            return good

        def zip_copy():
            assert D.zip_read_async(zt, ix.entries, count, None, count, 0, out, total, offsets, res, zwork, st) == 0

        def zip_copy_verify():
            assert D.zip_read_async(zt, ix.entries, count, None, count, D.DMX_ZIP_VERIFY, out, total, offsets, res, zwork, st) == 0

        def torch_copy():
            out.copy_(src)

        runs = {k: [] for k in ("torch_copy", "zip_copy", "zip_copy_verify")}
        oks = {}
        for _ in range(args.repeat):
            for k, fn in (("torch_copy", torch_copy), ("zip_copy", zip_copy), ("zip_copy_verify", zip_copy_verify)):
                runs[k].append(timed(fn))
                oks[k] = oks.get(k, True) and check()
        rec = {k: dict(figure(v), ok=oks[k], gb_s=round(total / min(v) / 1e6, 2)) for k, v in runs.items()}
        rec["zbytes"], rec["out_bytes"] = len(z), total
        rec["first_data_off_mod_16"] = int(ix.host["data_off"][0]) % 16
        rec["zip_copy_over_torch_copy"] = round(rec["zip_copy"]["ms"] / rec["torch_copy"]["ms"], 3)
        emit("stored", rec)


if __name__ == "__main__":
    main()
