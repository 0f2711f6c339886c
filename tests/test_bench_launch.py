"""bench.py's multi-rank plumbing on CPU: `--gpus N` without a launcher
starts N ranks itself, a world that differs from --gpus fails, and rank 0's stitched-stream
check (verify_stitched) accepts exactly the right stream.  The chunks here are shard streams
from the CPU oracle in the framing the HIP path emits."""
import json
import os
import subprocess
import sys
import zlib

import pytest

import deflate_compression_amd as D
from deflate_compression_amd import shard as S
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def _run(args, env_extra=None, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=180)


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_n_spawns_n_ranks(n):
    p = _run(["--gpus", str(n), "--launch-check"])
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == n and line["ranks_ok"]


def test_world_mismatch_exits_nonzero():
    p = _run(["--gpus", "2", "--launch-check"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2
    assert "launcher started 1 rank" in p.stderr


def test_steps_must_be_positive():
    p = _run(["--gpus", "1", "--steps", "0"])
    assert p.returncode == 2 and "--steps" in p.stderr


@pytest.mark.parametrize("size", [0, 5000, bench.DUMP_SAMPLE, bench.DUMP_SAMPLE + 4097])
def test_dump_outputs(tmp_path, size):
    """--dump-outputs: float arrays, a whole stream up to DUMP_SAMPLE bytes and a fixed sample
    beyond, chunk checksums over all of it, the same files for the same stream."""
    import numpy as np
    s = (np.arange(size, dtype=np.uint64) * 2654435761 >> 13).astype(np.uint8)
    res = D.Result(out_len=size, n=3 * size, adler=0xFFFFFFF1, status=0, nblocks=7)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    info = bench.dump_outputs(a, "", s, res)
    bench.dump_outputs(b, "_rank1", s.copy(), res)
    assert sorted(os.listdir(a)) == ["result.npy", "stream.npy", "stream_sums.npy"]
    got = {k: np.load(os.path.join(a, f"{k}.npy")) for k in ("result", "stream", "stream_sums")}
    for k, v in got.items():
        assert np.array_equal(v, np.load(os.path.join(b, f"{k}_rank1.npy")))
        assert list(v.shape) == info["arrays"][k]
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    rec = dict(zip(info["result_fields"], got["result"]))
    assert got["result"].dtype == np.float64 and rec["out_len"] == size and rec["adler"] == 0xFFFFFFF1
    assert rec["nblocks"] == 7 and rec["n"] == 3 * size
    assert got["stream"].dtype == np.float32 and info["stream_sampled"] == (size > bench.DUMP_SAMPLE)
    if size <= bench.DUMP_SAMPLE:
        assert np.array_equal(got["stream"], s.astype(np.float32))
    else:
        assert got["stream"].size == bench.DUMP_SAMPLE
        assert np.isin(got["stream"], s).all()
    sums = got["stream_sums"]
    assert sums.dtype == np.float64 and sums.shape == (-(-size // bench.DUMP_CHUNK), 2)
    assert sums[:, 0].sum() == int(s.sum(dtype=np.uint64))
    if size:   # the last (partial) chunk: plain and position-weighted sums
        tail = s[(sums.shape[0] - 1) * bench.DUMP_CHUNK:].astype(np.int64)
        assert sums[-1, 0] == tail.sum() and sums[-1, 1] == (tail * np.arange(1, tail.size + 1)).sum()
    if size > 1:   # one changed byte anywhere shows in its chunk's sums
        t = s.copy()
        t[size // 2] ^= 1
        c = str(tmp_path / "c")
        bench.dump_outputs(c, "", t, res)
        diff = np.load(os.path.join(c, "stream_sums.npy")) != sums
        assert diff.any(axis=1).sum() == 1 and diff[size // 2 // bench.DUMP_CHUNK].all()


def _shards(data: bytes, world: int, **kw):
    chunks, adlers, lens = [], [], []
    for r in range(world):
        lo, hi = S.shard_range(len(data), r, world)
        piece = data[lo:hi]
        chunks.append(O.compress(piece, flags=S.shard_flags(r, world), **kw))
        adlers.append(zlib.adler32(piece))
        lens.append(hi - lo)
    return chunks, adlers, lens


@pytest.mark.parametrize("world", [1, 2, 8])
def test_verify_stitched(world):
    data = D.gen_text(8 * 32768 + 777, 11).tobytes()
    chunks, adlers, lens = _shards(data, world, max_chain=6, lazy=True, store_check=True)
    bounds = [S.shard_range(len(data), r, world) for r in range(world)]
    pieces = [(lambda lo=lo, hi=hi: data[lo:hi]) for lo, hi in bounds]
    assert bench.verify_stitched(chunks, adlers, lens, pieces)
    # the one-stream framing: stitched == what zlib inflates to the input
    assert zlib.decompress(b"".join(chunks) + S.trailer(S.combine_adler(adlers, lens))) == data
    bad = bytearray(chunks[-1])
    bad[len(bad) // 2] ^= 0x10
    assert not bench.verify_stitched(chunks[:-1] + [bytes(bad)], adlers, lens, pieces)
    assert not bench.verify_stitched(chunks, [adlers[0] ^ 1] + adlers[1:], lens, pieces)
    if world > 1:   # a missing or a swapped chunk fails
        assert not bench.verify_stitched(chunks[1:], adlers, lens, pieces)
        assert not bench.verify_stitched(chunks[::-1], adlers, lens, pieces)
