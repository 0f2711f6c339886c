"""One .gz file of many members in one pass, the parts that need no GPU: the exports and their
declarations, every argument error of the three device calls (they return before any device call),
the work-size functions against csrc/dmx_pfind.h's layout arithmetic, the host plan of every input
of inflate_multi_inputs.py against zlib's member loop, and the plan with the member-bounded tail
rules under the sanitizers (tests/c/pmulti_model.cpp, a stand-alone program under ASan + UBSan)."""
import ctypes
import gzip
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import deflate_compression_amd as D
import inflate_multi_inputs as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = D.E
INVAL, RANGE = -E["E_INVAL"], -E["E_RANGE"]
CALLS = ("dmx_inflate_parallel_multi_plan_host", "dmx_inflate_parallel_multi_plan_work", "dmx_inflate_parallel_multi_plan_async",
         "dmx_inflate_parallel_multi_work", "dmx_inflate_parallel_multi_decode_async")
NAMES = ("PMember", "PMEMBER_DTYPE", "ParMultiStatus", "inflate_parallel_multi_plan_host", "inflate_parallel_multi_plan_async",
         "inflate_parallel_multi_decode_async", "inflate_parallel_multi")
A = 0x10000   # a 256-byte aligned address that is never dereferenced: the calls below return before any device call


def test_exports_and_declarations():
    L = D.lib()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in CALLS:
        f = getattr(L, name)
        assert f.argtypes is not None, name
        decl = re.search(r"^\w+\s+" + name + r"\(([^;]*?)\);", hdr, re.S | re.M).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(f.argtypes) == len([a for a in decl.split(",") if a.strip() not in ("", "void")]), name
    assert "One foreign file of many members" in hdr
    for name in NAMES:
        assert name in D.__all__ and getattr(D, name) is not None, name
        assert name in D.__doc__, name
    assert ctypes.sizeof(D.PMember) == 32 and ctypes.sizeof(D.ParMultiStatus) == 64 and ctypes.sizeof(D.PChunk) == 32
    assert np.dtype(D.PMEMBER_DTYPE).itemsize == 32
    assert re.search(r"uint32_t crc, isize; } dmx_pmember;", hdr) and re.search(r"nmembers, bad_member; } dmx_par_multi_status;", hdr)


def _a256(x):
    return (x + 255) & ~255


def _plan_bytes(nc):   # dmx_pf_mplan_bytes
    return 256 + _a256(32 * nc) + _a256(8 * nc) + _a256(32 * nc) + 8192 * min(nc, 1024) + _a256(8 * nc) + _a256(16 * nc)


def _work(out_len, nlive, nm):   # dmx_pf_mwork
    np_ = max(1, -(-out_len // 65536))
    return 256 + 8192 * min(max(nlive, 1), 2048) + _a256(2 * out_len) + _a256(4 * (nm + 1)) + _a256(4 * (np_ + nm))


def test_work_sizes():
    L = D.lib()
    prev = 0
    for zb in (0, 1, 1023, 1024, 1025, 100_000, 16384 * 1024, 16384 * 1024 + 1, 1 << 30, 0xFFFFFFF0):
        for chunk in (0, 1024, 4096, 65536, 1 << 30):
            nc = max(1, -(-zb // (chunk or 16384)))
            got = L.dmx_inflate_parallel_multi_plan_work(zb, chunk)
            assert got == _plan_bytes(nc) and got % 256 == 0, (zb, chunk, got)
        got = L.dmx_inflate_parallel_multi_plan_work(zb, 4096)
        assert got >= prev
        prev = got
    for chunk in (1, 1023, (1 << 30) + 1):
        assert L.dmx_inflate_parallel_multi_plan_work(1000, chunk) == 0
    assert L.dmx_inflate_parallel_multi_plan_work(0xFFFFFFF1, 0) == 0
    caps = (0, 1, 127, 128, 65535, 65536, 65537, 1 << 20, (100 << 20) + 3, 0xFFFFFFF0)
    lives = (0, 1, 2, 2047, 2048, 2049, 1 << 20)
    mems = (0, 1, 63, 64, 65, 25_000, 1 << 20)
    for nlive in lives:
        for nm in mems:
            prev = 0
            for cap in caps:
                got = L.dmx_inflate_parallel_multi_work(cap, nlive, nm)
                assert got == _work(cap, nlive, nm) and got % 256 == 0 and got >= prev, (cap, nlive, nm, got)
                prev = got
    for cap in caps:   # monotone in the other two
        for nm in mems:
            v = [L.dmx_inflate_parallel_multi_work(cap, nl, nm) for nl in lives]
            assert v == sorted(v)
        for nl in lives:
            v = [L.dmx_inflate_parallel_multi_work(cap, nl, nm) for nm in mems]
            assert v == sorted(v)
    a, b = M.two_sync()
    _, _, info = D.inflate_parallel_multi_plan_host(a + b, chunk_bytes=1024)
    assert info["work_len"] == L.dmx_inflate_parallel_multi_work(info["out_len"], info["nlive"], info["nmembers"])


def test_plan_argument_errors():
    plan = D.lib().dmx_inflate_parallel_multi_plan_async
    pb = D.lib().dmx_inflate_parallel_multi_plan_work(4000, 1024)
    assert plan(A, 4000, 0, 1024, None, pb, None) == INVAL          # d_plan NULL
    assert plan(None, 4000, 0, 1024, A, pb, None) == INVAL          # d_z NULL with bytes
    for fmt in (1, 3, 4):
        assert plan(A, 4000, fmt, 1024, A, pb, None) == INVAL       # zlib, raw, no format
    assert plan(A, 4000, 2, 1023, A, pb, None) == INVAL             # chunk_bytes
    assert plan(A, 4000, 0, (1 << 30) + 1, A, pb, None) == INVAL
    for mis in (1, 8, 128):
        assert plan(A, 4000, 0, 1024, A + mis, pb, None) == INVAL   # d_plan not 256-byte aligned
    assert plan(A, 4000, 0, 1024, A, pb - 1, None) == INVAL         # plan_bytes too small
    assert plan(A, 4000, 0, 1024, A, D.lib().dmx_inflate_parallel_plan_work(4000, 1024), None) == INVAL   # the single plan's size
    assert plan(A, 4000, 0, 1024, A, 0, None) == INVAL
    assert plan(A, 0xFFFFFFF1, 0, 1024, A, 1 << 40, None) == RANGE
    assert plan(A + 3, 0xFFFFFFF1, 2, 0, A, 1 << 40, None) == RANGE   # d_z may have any alignment


def test_decode_argument_errors():
    dec = D.lib().dmx_inflate_parallel_multi_decode_async
    pb = D.lib().dmx_inflate_parallel_multi_plan_work(4000, 1024)
    wb = D.lib().dmx_inflate_parallel_multi_work(10000, 4, 3)
    good = [A, 4000, A, pb, 4, 3, A, 10000, A, A, wb, 1, A, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return dec(*a)

    assert call(a0=None) == INVAL          # d_z NULL with bytes
    assert call(a2=None) == INVAL          # d_plan
    assert call(a6=None) == INVAL          # d_out NULL with a capacity
    assert call(a8=None) == INVAL          # d_members NULL with a capacity
    assert call(a9=None) == INVAL          # d_work
    assert call(a12=None) == INVAL         # d_status
    for mis in (1, 8, 128):
        assert call(a2=A + mis) == INVAL   # d_plan, d_work: 256 bytes
        assert call(a9=A + mis) == INVAL
    for mis in (1, 2, 4):
        assert call(a12=A + mis) == INVAL  # d_status, d_members: 8 bytes
        assert call(a8=A + mis) == INVAL
    assert call(a3=D.lib().dmx_inflate_parallel_multi_plan_work(1, 0) - 1) == INVAL   # less than the smallest plan
    assert call(a3=0) == INVAL
    assert call(a10=255) == INVAL          # less than the control block
    assert call(a1=0xFFFFFFF1) == RANGE
    assert call(a0=A + 1, a1=0xFFFFFFF1) == RANGE   # d_z may have any alignment


def test_host_plan_argument_errors():
    z = M.single()
    for fmt in ("zlib", "raw"):
        rec = D.ParMultiStatus()
        assert D.lib().dmx_inflate_parallel_multi_plan_host(z, len(z), D._BATCH_FMT[fmt], 1024, None, 0, None, 0,
                                                            ctypes.byref(rec)) == INVAL
    rec = D.ParMultiStatus()
    assert D.lib().dmx_inflate_parallel_multi_plan_host(z, len(z), 0, 1023, None, 0, None, 0, ctypes.byref(rec)) == INVAL
    assert D.lib().dmx_inflate_parallel_multi_plan_host(z, len(z), 0, 1024, None, 0, None, 0, None) == INVAL
    for bad in (b"\x78\x9c" + z, b"", b"\x1f"):
        _, _, info = D.inflate_parallel_multi_plan_host(bad, chunk_bytes=1024)
        assert info["status"] == -E["E_ZHEAD"] and info["nmembers"] == 0, info


def check_plan(z, chunks, members, info):
    """the host plan against zlib's member loop: the member table, the chunks' tiling and chain"""
    ref, used = M.reference(z)
    assert info["status"] == 0 and info["gave_up"] == 0, info
    assert info["nmembers"] == len(ref) == len(members) and info["in_used"] == used
    assert info["out_len"] == sum(r[1] for r in ref) and info["check"] == ref[-1][2]
    assert info["bad_member"] == 0xFFFFFFFF and info["nlive"] == len(chunks) and info["ndead"] == info["ncand"] - info["nlive"]
    off = 0
    for k, (in_off, n, crc, _) in enumerate(ref):
        m = members[k]
        assert (int(m["in_off"]), int(m["out_off"]), int(m["out_len"]), int(m["crc"]), int(m["isize"])) == \
            (in_off, off, n, crc, n & 0xFFFFFFFF), k
        off += n
    # chunk 0 begins at the first header; end_bit of one is bit of the next -- a chunk that ends with a
    # member ends at the next member's first byte, behind alignment and trailer; the last one ends with
    # the last block, in front of alignment and trailer
    assert int(chunks["bit"][0]) == 0 and int(chunks["out_off"][0]) == 0
    assert np.array_equal(chunks["out_off"][1:], np.cumsum(chunks["out_len"])[:-1].astype(np.uint64))
    assert int(chunks["out_len"].sum()) == info["out_len"]
    assert np.array_equal(chunks["bit"][1:], chunks["end_bit"][:-1])
    assert np.all(chunks["bit"] < chunks["end_bit"])
    assert ((int(chunks["end_bit"][-1]) + 7) >> 3) + 8 == used
    starts = {8 * r[0] for r in ref}
    for k in range(1, len(chunks)):
        bit = int(chunks["bit"][k])
        if bit & 7 == 0 and z[bit >> 3] == 0x1F:   # the chunk begins at a header: a member of the file's
            assert bit in starts, (k, bit)


@pytest.mark.parametrize("name,z", M.well_formed() + M.trailing(), ids=lambda v: v if isinstance(v, str) else "")
def test_host_plan(name, z):
    for chunk in (1024, 4096):
        chunks, members, info = D.inflate_parallel_multi_plan_host(z, chunk_bytes=chunk)
        check_plan(z, chunks, members, info)
    ref, used = M.reference(z)
    if used == len(z):
        assert gzip.decompress(z) == b"".join(r[3] for r in ref)


def test_host_plan_conditions():
    """what the GPU tests rely on: small-300 has many live chunks that begin at member starts (its
    blocks are all final: the block search finds nothing in it); single equals the single-stream
    plan; the false member starts of header-straddle and nested are candidates, and dead"""
    z = M.small_300()
    chunks, members, info = D.inflate_parallel_multi_plan_host(z, chunk_bytes=1024)
    assert info["nlive"] > 8 and info["gave_up"] == 0 and info["nmembers"] == 300, info
    assert all(int(b) & 7 == 0 and z[int(b) >> 3] == 0x1F for b in chunks["bit"])
    assert 700 <= int(members["out_len"].min()) and int(members["out_len"].max()) <= 3000
    z = M.single()
    chunks, members, info = D.inflate_parallel_multi_plan_host(z, chunk_bytes=1024)
    c1, i1 = D.inflate_parallel_plan_host(z, chunk_bytes=1024)
    assert info["nmembers"] == 1 and info["nlive"] == i1["nlive"] > 8
    for f in ("status", "format", "out_len", "in_used", "check", "nchunks", "ncand", "nlive", "ndead", "gave_up"):
        assert info[f] == i1[f], f
    assert np.array_equal(chunks[1:], c1[1:]) and int(c1["bit"][0]) == 80 and int(chunks["end_bit"][0]) == int(c1["end_bit"][0])
    for z, at in ((M.header_straddle(), None), (M.nested(), 8 * M.CHUNK)):
        chunks, members, info = D.inflate_parallel_multi_plan_host(z, chunk_bytes=1024)
        assert info["ndead"] >= (2 if at is None else 1), info
        if at is not None:
            assert at not in set(int(b) for b in chunks["bit"])
    z = M.header_straddle()
    chunks, members, info = D.inflate_parallel_multi_plan_host(z, chunk_bytes=1024)
    for m in members[1:3]:   # both padded headers span a chunk boundary
        p = int(m["in_off"])
        assert p // 1024 != (p + 12 + int.from_bytes(z[p + 10:p + 12], "little")) // 1024


def test_host_plan_serial_route_input():
    z = M.five_mib_zeros()
    chunks, members, info = D.inflate_parallel_multi_plan_host(z, chunk_bytes=1024)
    assert info["status"] == -E["E_RANGE"] and info["gave_up"] == 1 and info["out_len"] == 0, info
    ref, used = M.reference(z)
    assert len(ref) == 3 and ref[1][1] == 5 << 20 and used == len(z) < 1_000_000


def test_host_plan_statuses():
    for name, z, plan_status, _, _ in M.broken():
        with pytest.raises(zlib.error):
            M.reference(z)
        _, _, info = D.inflate_parallel_multi_plan_host(z, chunk_bytes=1024)
        if plan_status is None:
            assert info["status"] == -E["E_LEN"], (name, info)   # the block's status: its input ends
        else:
            assert info["status"] == plan_status, (name, info)
        if info["status"]:
            assert info["out_len"] == 0 and info["in_used"] == 0 and info["nmembers"] == 0
    for name, z, off, bit in M.far_files():
        with pytest.raises(zlib.error, match="too far back"):
            M.reference(z)
        chunks, members, info = D.inflate_parallel_multi_plan_host(z, chunk_bytes=1024)
        assert info["status"] == 0 and info["nlive"] >= 2 and info["nmembers"] == 2, (name, info)   # distances are the decode's
        assert int(members["in_off"][1]) == off and off % 1024 > 64
        if name == "far-b":   # a live chunk starts with the bad block, less than 32 768 bytes into member 1
            k = list(chunks["bit"]).index(bit)
            assert k >= 2 and 0 < int(chunks["out_off"][k]) - int(members["out_off"][1]) < 32768


def test_plan_and_rules_asan_ubsan(tmp_path):
    """tests/c/pmulti_model.cpp ends with `0 failed checks`: the host plan of every input at two chunk
    sizes and of every truncation of empties and header-straddle, and the member-bounded pack and
    tail rules, through the headers the kernels compile."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "-f", "Makefile.pmulti"])
    exe = os.path.join(REPO, "build", "c", "pmulti_model")

    def put(name, z):
        p = tmp_path / name
        p.write_bytes(z)
        return str(p)

    plain = [put(n, z) for n, z in M.well_formed() + M.trailing()] + [put(b[0], b[1]) for b in M.broken()] + \
        [put(f[0], f[1]) for f in M.far_files()] + [put("five-mib-zeros", M.five_mib_zeros())]
    cut = [put("cut-empties", M.empties()), put("cut-header-straddle", M.header_straddle())]
    p = subprocess.run([exe] + plain + ["-t"] + cut, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    m = re.search(r"(\d+) checks, 0 failed checks", p.stdout)
    assert m and int(m.group(1)) > 50_000, p.stdout[-500:]
