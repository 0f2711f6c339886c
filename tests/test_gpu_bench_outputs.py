"""A plain bench.py run (no --full) with --dump-outputs, as a child process: the line carries the
headline figures only, and the dumped arrays are the last timed step's zlib stream of the seeded
input (whole here: 1 MB of text compresses well below the sample size) and its result record."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import deflate_compression_amd as D

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

N = 1_000_003   # not a multiple of the 32 KiB block


def test_plain_run_dumps_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--bytes", str(N), "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["full"] is False and line["steps"] == 2 and line["warmup"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # both are rounded (3 and 4 decimals): 1 % covers a step as short as 0.005 ms
    assert line["value"] == pytest.approx(N / line["ms_per_step"] / 1e6, rel=1e-2)
    for k in ("stage_ms", "roofline", "gpu_inflate", "cpu_baseline", "tradeoff", "exhaustive", "long_run"):
        assert k not in line   # --full only
    assert sorted(os.listdir(out)) == ["result.npy", "stream.npy", "stream_sums.npy"]
    res = np.load(out / "result.npy")
    stream = np.load(out / "stream.npy")
    sums = np.load(out / "stream_sums.npy")
    assert res.dtype == np.float64 and stream.dtype == np.float32 and sums.dtype == np.float64
    fields = dict(zip(line["outputs"]["result_fields"], res))
    assert fields["out_len"] == stream.size == line["compressed_bytes_rank0"] and fields["n"] == N
    assert fields["status"] == 0 and fields["nblocks"] == -(-N // 32768)
    data = D.gen_text(N, bench.WORKLOADS["text"][2]).tobytes()
    z = stream.astype(np.uint8).tobytes()
    assert zlib.decompress(z) == data
    assert fields["adler"] == zlib.adler32(data)
    assert sums[:, 0].sum() == sum(z)
    assert sums.shape == (-(-len(z) // bench.DUMP_CHUNK), 2)
