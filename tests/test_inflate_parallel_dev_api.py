"""One foreign stream decoded in one pass on the device, the parts that need no GPU: the exports and
their declarations, every argument error of dmx_inflate_parallel_plan_async and
dmx_inflate_parallel_decode_async (they return before any device call), the work-size functions
against csrc/dmx_pfind.h's layout arithmetic, the host plan of the new crafted streams, and the tail
and pack rules under the sanitizers (tests/c/ptail_model.cpp: csrc/dmx_ptail.h, the text the kernels
run, in a stand-alone program under ASan + UBSan)."""
import ctypes
import os
import re
import subprocess

import numpy as np

import deflate_compression_amd as D
import inflate_parallel_dev_inputs as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE = -E["E_INVAL"], -E["E_RANGE"]
CALLS = ("dmx_inflate_parallel_plan_work", "dmx_inflate_parallel_plan_async", "dmx_inflate_parallel_work",
         "dmx_inflate_parallel_decode_async")
A = 0x10000   # a 256-byte aligned address that is never dereferenced: the calls below return before any device call


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in CALLS:
        f = getattr(L, name)
        assert f.argtypes is not None, name
        assert name + "(" in hdr, name
        decl = re.search(r"^\w+\s+" + name + r"\(([^;]*?)\);", hdr, re.S | re.M).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(f.argtypes) == len([a for a in decl.split(",") if a.strip() not in ("", "void")]), name
    assert "One foreign stream: the decode" in hdr
    for name in ("inflate_parallel", "inflate_parallel_plan_async", "inflate_parallel_decode_async"):
        assert name in D.__all__ and callable(getattr(D, name)), name


def _a256(x):
    return (x + 255) & ~255


def _plan_bytes(nc):   # dmx_pf_plan_bytes
    return 256 + _a256(32 * nc) + _a256(8 * nc) + _a256(32 * nc) + 8192 * min(nc, 1024)


def _work(out_len, nlive):   # dmx_pf_work
    np_ = max(1, -(-out_len // 65536))
    return 256 + 8192 * min(max(nlive, 1), 2048) + _a256(2 * out_len) + _a256(24 * np_) + 2 * _a256(4 * np_)


def test_work_sizes():
    L = D.lib()
    prev = 0
    for zb in (0, 1, 1023, 1024, 1025, 100_000, 16384 * 1024, 16384 * 1024 + 1, 1 << 30, 0xFFFFFFF0):
        for chunk in (0, 1024, 4096, 65536, 1 << 30):
            nc = max(1, -(-zb // (chunk or 16384)))
            got = L.dmx_inflate_parallel_plan_work(zb, chunk)
            assert got == _plan_bytes(nc) and got % 256 == 0, (zb, chunk, got)
        got = L.dmx_inflate_parallel_plan_work(zb, 4096)
        assert got >= prev
        prev = got
    for chunk in (1, 1023, (1 << 30) + 1):
        assert L.dmx_inflate_parallel_plan_work(1000, chunk) == 0
    assert L.dmx_inflate_parallel_plan_work(0xFFFFFFF1, 0) == 0
    for nlive in (0, 1, 2, 2047, 2048, 2049, 1 << 20):
        prev = 0
        for cap in (0, 1, 127, 128, 65535, 65536, 65537, 1 << 20, (100 << 20) + 3, 0xFFFFFFF0):
            got = L.dmx_inflate_parallel_work(cap, nlive)
            assert got == _work(cap, nlive) and got % 256 == 0 and got >= prev, (cap, nlive, got)
            prev = got
    assert L.dmx_inflate_parallel_work(1000, 5) <= L.dmx_inflate_parallel_work(1000, 6)
    # the record of the host plan names the same number
    z, _ = P.run_stream()
    chunks, info = D.inflate_parallel_plan_host(z, chunk_bytes=1024)
    assert info["work_len"] == L.dmx_inflate_parallel_work(info["out_len"], info["nlive"])


def test_plan_argument_errors():
    plan = D.lib().dmx_inflate_parallel_plan_async
    pb = D.lib().dmx_inflate_parallel_plan_work(4000, 1024)
    assert plan(A, 4000, 0, 1024, None, pb, None) == INVAL          # d_plan NULL
    assert plan(None, 4000, 0, 1024, A, pb, None) == INVAL          # d_z NULL with bytes
    assert plan(A, 4000, 4, 1024, A, pb, None) == INVAL             # fmt
    assert plan(A, 4000, 0, 1023, A, pb, None) == INVAL             # chunk_bytes
    assert plan(A, 4000, 0, (1 << 30) + 1, A, pb, None) == INVAL
    for mis in (1, 8, 128):
        assert plan(A, 4000, 0, 1024, A + mis, pb, None) == INVAL   # d_plan not 256-byte aligned
    assert plan(A, 4000, 0, 1024, A, pb - 1, None) == INVAL         # plan_bytes too small
    assert plan(A, 4000, 0, 1024, A, 0, None) == INVAL
    assert plan(A, 0xFFFFFFF1, 0, 1024, A, 1 << 40, None) == RANGE
    assert plan(A + 3, 0xFFFFFFF1, 3, 0, A, 1 << 40, None) == RANGE   # d_z may have any alignment


def test_decode_argument_errors():
    dec = D.lib().dmx_inflate_parallel_decode_async
    pb = D.lib().dmx_inflate_parallel_plan_work(4000, 1024)
    wb = D.lib().dmx_inflate_parallel_work(10000, 4)
    good = [A, 4000, A, pb, 4, A, 10000, A, wb, 1, A, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return dec(*a)

    assert call(a0=None) == INVAL          # d_z NULL with bytes
    assert call(a2=None) == INVAL          # d_plan
    assert call(a5=None) == INVAL          # d_out NULL with a capacity
    assert call(a7=None) == INVAL          # d_work
    assert call(a10=None) == INVAL         # d_status
    for mis in (1, 8, 128):
        assert call(a2=A + mis) == INVAL   # d_plan, d_work: 256 bytes
        assert call(a7=A + mis) == INVAL
    for mis in (1, 2, 4):
        assert call(a10=A + mis) == INVAL  # d_status: 8 bytes
    assert call(a3=D.lib().dmx_inflate_parallel_plan_work(1, 0) - 1) == INVAL   # less than the smallest plan
    assert call(a3=0) == INVAL
    assert call(a8=255) == INVAL           # less than the control block
    assert call(a1=0xFFFFFFF1) == RANGE
    assert call(a0=A + 1, a1=0xFFFFFFF1) == RANGE   # d_z may have any alignment


def test_host_plan_of_the_run_stream():
    """the numbers the GPU tests rely on, from the host plan: several chunks in front of the run block,
    one long chunk that begins at or just in front of it, several behind it"""
    z, data = P.run_stream()
    chunks, info = D.inflate_parallel_plan_host(z, chunk_bytes=1024)
    assert info["status"] == 0 and info["gave_up"] == 0 and info["out_len"] == len(data), info
    assert info["nlive"] >= 12 and len(data) > 130_000
    long_ = [k for k in range(len(chunks)) if int(chunks["out_len"][k]) > 65536]
    assert len(long_) == 1
    k = long_[0]
    assert P.RUN_OFF - 32768 <= int(chunks["out_off"][k]) <= P.RUN_OFF
    assert k >= 4 and len(chunks) - 1 - k >= 4
    for name, z, off in P.too_far_streams():
        chunks, info = D.inflate_parallel_plan_host(z, chunk_bytes=1024)
        assert info["status"] == 0, (name, info)   # distances are the decode's to find
        k = int(np.searchsorted(chunks["out_off"], off, side="right")) - 1
        assert (k == 0) == (name == "first-block") and int(chunks["out_off"][k]) < 32768, (name, k)


def test_tail_rules_asan_ubsan():
    """tests/c/ptail_model.cpp ends with `0 failed checks`: random token streams cut at random chunk
    starts (chunk lengths 1, 100, 32 767, 32 768, 32 769, 70 000 in every order of two; distances
    32 768 and 32 767 across one and several chunk starts; windows assembled from up to 40 short
    chunks; a chunk whose last 32 768 cells are all references; references before output offset 0)
    resolve to the bytes of a plain decode through the header the kernels compile."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.ptail"])
    exe = os.path.join(REPO, "build", "c", "ptail_model")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    m = re.search(r"(\d+) checks, 0 failed checks", p.stdout)
    assert m and int(m.group(1)) > 1_000_000, p.stdout[-500:]
