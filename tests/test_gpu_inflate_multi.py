"""One .gz file of many members decoded in one pass on the device
(dmx_inflate_parallel_multi_plan_async, dmx_inflate_parallel_multi_decode_async,
inflate_parallel_multi): the device plan against the host plan, the decode and the member table
against zlib's member loop (inflate_multi_inputs.reference), the statuses, the two-call idiom with
canaries, unaligned input, a captured graph, three chunk sizes.  chunk_bytes is 1 024 unless said.
The bounded cases come first in file order; the serial-route case runs behind them, and only when
all of those passed."""
import functools
import gzip

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
import inflate_multi_inputs as M

pytestmark = pytest.mark.gpu

E = D.E
SZ, RANGE, HUFDIS = -E["E_SZ"], -E["E_RANGE"], -E["E_HUFDIS"]
CANARY = 0xA5
GUARD = 64
NOBAD = 0xFFFFFFFF

_bounded = {}   # bounded case -> passed; the unbounded case runs when every one of them did


def bounded(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        key = (fn.__name__, tuple(a), tuple(sorted(kw.items())))
        _bounded[key] = False
        fn(*a, **kw)
        _bounded[key] = True
    return run


def need_bounded():
    if not _bounded or not all(_bounded.values()):
        pytest.skip("bounded cases did not pass")


FILES = dict(M.well_formed() + M.trailing())
BROKEN = {b[0]: b for b in M.broken()}
FAR = {f[0]: f for f in M.far_files()}
_refs = {}


def ref_of(name):
    if name not in _refs:
        _refs[name] = M.reference(FILES[name])
    return _refs[name]


def on_device(z, shift=0):
    """z in device memory, `shift` bytes above the start of its allocation"""
    buf = torch.zeros(len(z) + shift + 8, dtype=torch.uint8, device="cuda")
    buf[shift:shift + len(z)] = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    return buf[shift:shift + len(z)]


def record(t):
    return D.ParMultiStatus.from_buffer_copy(t.cpu().numpy().tobytes()[:64])


def fields(rec):
    d = {f: int(getattr(rec.st, f)) for f, _ in D.ParStatus._fields_}
    d["nmembers"], d["bad_member"] = int(rec.nmembers), int(rec.bad_member)
    return d


def plan_dev(zt, chunk=1024):
    pb = D.lib().dmx_inflate_parallel_multi_plan_work(zt.numel(), chunk)
    assert pb and pb % 256 == 0
    plan = torch.full((pb,), 0x5A, dtype=torch.uint8, device="cuda")
    assert D.inflate_parallel_multi_plan_async(zt, D.DMX_BATCH_GZIP, chunk, plan) == 0
    rec = record(plan[:64])
    chunks = plan[256:256 + 32 * rec.st.nlive].cpu().numpy().view(D.PCHUNK_DTYPE) if rec.st.nlive <= rec.st.nchunks else None
    return plan, rec, chunks


def same_plan(z, chunk, rec, chunks, what):
    """the 64-byte record and the live chunks equal the host plan's, field for field (behind a status
    the failing chunk's end_bit and out_len are where its decode stopped: unspecified)"""
    hc, hm, hi = D.inflate_parallel_multi_plan_host(z, chunk_bytes=chunk)
    assert fields(rec) == hi, (what, fields(rec), hi)
    assert chunks is not None and len(chunks) == len(hc), what
    n = len(hc) - (1 if hi["status"] else 0)
    assert chunks[:n].tobytes() == hc[:n].tobytes(), what
    if hi["status"] and len(hc):
        assert (int(chunks["bit"][-1]), int(chunks["out_off"][-1])) == (int(hc["bit"][-1]), int(hc["out_off"][-1])), what
    return hi, hm


def decode_dev(zt, plan, max_live, max_members, out_cap, work_bytes, verify=True):
    """-> (record, guarded output, guarded member table as bytes)"""
    big = torch.full((out_cap + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    mem = torch.full((32 * max_members + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    work = torch.empty(max(work_bytes, 256), dtype=torch.uint8, device="cuda")
    st = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    r = D.inflate_parallel_multi_decode_async(zt, plan, max_live, max_members, big[GUARD:GUARD + out_cap] if out_cap else None,
                                              out_cap, mem[GUARD:GUARD + 32 * max_members] if max_members else None,
                                              work[:work_bytes], verify, st)
    assert r == 0
    return record(st), big.cpu().numpy(), mem.cpu().numpy()


def untouched(big, lo=0):
    """every byte of a guarded buffer from payload position lo on still holds the canary"""
    return bool((big[:GUARD] == CANARY).all() and (big[GUARD + lo:] == CANARY).all())


def members_of(mem, n):
    return mem[GUARD:GUARD + 32 * n].view(D.PMEMBER_DTYPE)


def check_members(members, ref):
    off = 0
    assert len(members) == len(ref)
    for k, (in_off, n, crc, _) in enumerate(ref):
        m = members[k]
        assert (int(m["in_off"]), int(m["out_off"]), int(m["out_len"]), int(m["crc"]), int(m["isize"])) == \
            (in_off, off, n, crc, n & 0xFFFFFFFF), k
        off += n


def check_decode(name, z, ref, used, chunk=1024, shift=0, verify=True, slack=0):
    zt = on_device(z, shift)
    plan, rec, chunks = plan_dev(zt, chunk)
    hi, hm = same_plan(z, chunk, rec, chunks, name)
    assert hi["status"] == 0 and hi["in_used"] == used
    data = b"".join(r[3] for r in ref)
    cap, ml, mm = hi["out_len"] + slack, hi["nlive"] + (3 if slack else 0), hi["nmembers"] + (2 if slack else 0)
    wb = D.lib().dmx_inflate_parallel_multi_work(cap, ml, mm) if slack else hi["work_len"]
    got, big, mem = decode_dev(zt, plan, ml, mm, cap, wb, verify)
    assert fields(got) == hi, (name, fields(got), hi)
    assert big[GUARD:GUARD + len(data)].tobytes() == data, name
    assert untouched(big, len(data)), name             # nothing behind out_len, nothing behind out_cap
    assert untouched(mem, 32 * hi["nmembers"]), name   # no record behind nmembers
    check_members(members_of(mem, hi["nmembers"]), ref)
    assert members_of(mem, hi["nmembers"]).tobytes() == hm.tobytes()   # the host plan's table is the model
    return hi


# ---- bounded: plan and decode of every input ------------------------------------------------------
@pytest.mark.parametrize("name", list(FILES))
@bounded
def test_plan_and_decode(name):
    z = FILES[name]
    ref, used = ref_of(name)
    hi = check_decode(name, z, ref, used)
    assert hi["nlive"] > 1
    if used == len(z):
        assert gzip.decompress(z) == b"".join(r[3] for r in ref)
    else:
        assert used == len(b"".join(M.two_sync()))   # trailing data is ignored


@pytest.mark.parametrize("chunk", [1024, 4096, 65536])
@bounded
def test_small_300_at_three_chunk_sizes(chunk):
    ref, used = ref_of("small-300")
    hi = check_decode("small-300", FILES["small-300"], ref, used, chunk=chunk)
    assert hi["nmembers"] == 300 and hi["nlive"] >= 4


@pytest.mark.parametrize("shift", [1, 2, 3])
@bounded
def test_unaligned_input_and_larger_capacities(shift):
    for name in ("two-sync", "header-straddle"):
        ref, used = ref_of(name)
        check_decode(name, FILES[name], ref, used, shift=shift, slack=1000 + shift)


@bounded
def test_single_equals_inflate_parallel():
    z = FILES["single"]
    info, info1 = {}, {}
    out, members = D.inflate_parallel_multi(on_device(z), chunk_bytes=1024, info=info)
    out1 = D.inflate_parallel(on_device(z), chunk_bytes=1024, info=info1)
    assert info["route"] == info1["route"] == "parallel" and info["nmembers"] == 1 and len(members) == 1
    assert torch.equal(out, out1)
    for f in ("status", "format", "out_len", "in_used", "check", "nchunks", "ncand", "nlive", "ndead", "gave_up"):
        assert info[f] == info1[f], f
    check_members(members, ref_of("single")[0])


# ---- bounded: statuses ----------------------------------------------------------------------------
def _status_of(z, verify=True):
    zt = on_device(z)
    plan, rec, chunks = plan_dev(zt)
    hi, _ = same_plan(z, 1024, rec, chunks, "status")
    ml, mm, cap = max(rec.st.nchunks, 1), 8, 200_000
    if rec.st.status == 0:
        ml, mm, cap = rec.st.nlive, rec.nmembers, rec.st.out_len
    got, big, mem = decode_dev(zt, plan, ml, mm, cap, D.lib().dmx_inflate_parallel_multi_work(cap, ml, mm), verify)
    if rec.st.status:
        assert fields(got) == fields(rec) and untouched(big) and untouched(mem)   # nothing is decoded
    else:
        assert untouched(big, rec.st.out_len) and untouched(mem, 32 * rec.nmembers)
    if got.st.status:
        assert (got.st.out_len, got.st.in_used, got.st.check, got.st.work_len) == (0, 0, 0, 0)
    return rec, got, big


@pytest.mark.parametrize("name", list(BROKEN))
@bounded
def test_broken_ends(name):
    _, z, plan_status, status, bad = BROKEN[name]
    rec, got, big = _status_of(z)
    if plan_status is None:   # cut in a block: the block's status, the host plan's (same_plan)
        assert rec.st.status == got.st.status == -E["E_LEN"]
    else:
        assert (rec.st.status, got.st.status) == (plan_status, status), name
    assert got.bad_member == (NOBAD if bad is None else bad)
    if bad is not None:   # a wrong CRC-32 or ISIZE: clean without verify, the bytes are all there
        rec, got, big = _status_of(z, verify=False)
        data = b"".join(r[3] for r in ref_of("two-sync")[0])
        assert got.st.status == 0 and got.bad_member == NOBAD and big[GUARD:GUARD + len(data)].tobytes() == data


@bounded
def test_the_first_bad_member_is_named():
    a, b = M.two_sync()
    z = bytearray(a + b + a)
    z[len(a) - 8] ^= 1               # member 0's CRC-32
    z[len(a) + len(b) - 4] ^= 1      # member 1's ISIZE
    rec, got, _ = _status_of(bytes(z))
    assert (got.st.status, got.bad_member) == (-E["E_CRC"], 0)
    z[len(a) - 8] ^= 1
    rec, got, _ = _status_of(bytes(z))
    assert (got.st.status, got.bad_member) == (-E["E_LEN"], 1)
    z[len(a) + len(b) - 8] ^= 1      # both of member 1: the CRC-32 is checked first
    rec, got, _ = _status_of(bytes(z))
    assert (got.st.status, got.bad_member) == (-E["E_CRC"], 1)


@pytest.mark.parametrize("name", list(FAR))
@bounded
def test_a_distance_before_the_member(name):
    _, z, off, bit = FAR[name]
    rec, got, _ = _status_of(z)
    assert rec.st.status == 0 and rec.st.nlive >= 2 and got.st.status == HUFDIS, (name, got.st.status)
    assert got.bad_member == NOBAD
    with pytest.raises(D.DeflateError) as e:   # the same member alone, through the host decoder
        D.deflate_decompress(z[off:])
    assert e.value.code == HUFDIS


# ---- bounded: the two-call idiom ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two-sync", "small-300"])
@bounded
def test_capacities_one_short(name):
    z = FILES[name]
    zt = on_device(z)
    plan, rec, _ = plan_dev(zt)
    s = rec.st
    assert s.status == 0 and s.nlive > 1 and rec.nmembers > 1
    exact = (s.nlive, rec.nmembers, s.out_len, s.work_len)
    for what, k in (("max_live", 0), ("max_members", 1), ("out_cap", 2), ("work_bytes", 3)):
        a = list(exact)
        a[k] -= 256 if k == 3 else 1
        got, big, mem = decode_dev(zt, plan, *a)
        assert got.st.status == SZ, (what, got.st.status)
        assert (got.st.nlive, got.nmembers, got.st.out_len, got.st.work_len) == exact, what
        assert untouched(big) and untouched(mem), what
    got, big, mem = decode_dev(zt, plan, *exact)   # and the exact numbers pass
    data = b"".join(r[3] for r in ref_of(name)[0])
    assert got.st.status == 0 and big[GUARD:GUARD + len(data)].tobytes() == data
    assert untouched(big, len(data)) and untouched(mem, 32 * rec.nmembers)


# ---- bounded: in a graph --------------------------------------------------------------------------
@bounded
def test_plan_and_decode_in_a_graph():
    """plan + decode captured once with capacities, replayed on two-sync and on a second file of the
    same length written into the same tensor"""
    za = FILES["two-sync"]
    t = M.text()
    parts = [M.member(t[300_000 + 9000 * k:300_000 + 9000 * (k + 1)], flush_every=2000) for k in range(8)]
    zb = b"".join(parts)
    assert len(zb) < len(za) - 18
    zb += bytes(len(za) - len(zb))   # zero padding behind the last trailer is ignored
    refs = {za: ref_of("two-sync"), zb: M.reference(zb)}
    assert len(refs[zb][0]) == 8
    n, chunk, cap, mm = len(za), 1024, 130_000, 10
    L = D.lib()
    nc = -(-n // chunk)
    zt = torch.zeros(n, dtype=torch.uint8, device="cuda")
    plan = torch.zeros(L.dmx_inflate_parallel_multi_plan_work(n, chunk), dtype=torch.uint8, device="cuda")
    work = torch.zeros(L.dmx_inflate_parallel_multi_work(cap, nc, mm), dtype=torch.uint8, device="cuda")
    big = torch.zeros(cap + 2 * GUARD, dtype=torch.uint8, device="cuda")
    mem = torch.zeros(32 * mm + 2 * GUARD, dtype=torch.uint8, device="cuda")
    st = torch.zeros(8, dtype=torch.int64, device="cuda")

    def enqueue():
        r = D.inflate_parallel_multi_plan_async(zt, 0, chunk, plan)
        return r or D.inflate_parallel_multi_decode_async(zt, plan, nc, mm, big[GUARD:GUARD + cap], cap,
                                                          mem[GUARD:GUARD + 32 * mm], work, True, st)

    zt.copy_(torch.frombuffer(bytearray(za), dtype=torch.uint8))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the kernels are loaded before the capture
        assert enqueue() == 0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r = enqueue()
    assert r == 0
    for z in (za, zb, za):
        ref, used = refs[z]
        data = b"".join(r[3] for r in ref)
        zt.copy_(torch.frombuffer(bytearray(z), dtype=torch.uint8))
        big.fill_(CANARY)
        mem.fill_(CANARY)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = record(st)
        assert (got.st.status, got.nmembers, got.st.out_len, got.st.in_used) == (0, len(ref), len(data), used)
        h, hm = big.cpu().numpy(), mem.cpu().numpy()
        assert h[GUARD:GUARD + len(data)].tobytes() == data and untouched(h, len(data))
        check_members(members_of(hm, len(ref)), ref)
        assert untouched(hm, 32 * len(ref))


# ---- the Python route -----------------------------------------------------------------------------
@bounded
def test_inflate_parallel_multi():
    for name in ("two-sync", "empties", "junk-behind"):
        ref, used = ref_of(name)
        info = {}
        out, members = D.inflate_parallel_multi(FILES[name], chunk_bytes=1024, info=info)   # bytes
        assert info["route"] == "parallel" and info["status"] == 0 and info["in_used"] == used, (name, info)
        assert out.cpu().numpy().tobytes() == b"".join(r[3] for r in ref)
        check_members(members, ref)
    info = {}
    out, members = D.inflate_parallel_multi(on_device(FILES["small-300"]), info=info)   # the default cut
    assert info["route"] == "parallel" and info["nmembers"] == 300
    assert out.cpu().numpy().tobytes() == b"".join(r[3] for r in ref_of("small-300")[0])
    with pytest.raises(D.DeflateError, match="member 1") as e:
        D.inflate_parallel_multi(BROKEN["crc-flip"][1], chunk_bytes=1024)
    assert e.value.code == -E["E_CRC"]
    out, _ = D.inflate_parallel_multi(BROKEN["crc-flip"][1], chunk_bytes=1024, verify=False)
    assert out.numel() == 120_000
    with pytest.raises(D.DeflateError) as e:
        D.inflate_parallel_multi(BROKEN["method-7"][1], chunk_bytes=1024)
    assert e.value.code == -E["E_ZCMPMT"]
    with pytest.raises(D.DeflateError) as e:
        D.inflate_parallel_multi(b"\x78\x9c" + FILES["single"], chunk_bytes=1024)
    assert e.value.code == -E["E_ZHEAD"]


# ---- unbounded: behind the bounded cases, and only when they all passed ---------------------------
def test_five_mib_of_zeros_take_the_serial_route():
    need_bounded()
    z = M.five_mib_zeros()
    ref, used = M.reference(z)
    info = {}
    out, members = D.inflate_parallel_multi(z, chunk_bytes=1024, info=info)
    assert info["route"] == "serial" and info["gave_up"] == 1 and info["nmembers"] == 3 and info["in_used"] == used
    assert out.cpu().numpy().tobytes() == b"".join(r[3] for r in ref)
    check_members(members, ref)
    bad = bytearray(z)
    bad[int(members["in_off"][2]) - 8] ^= 1   # member 1's CRC-32
    with pytest.raises(D.DeflateError, match="member 1") as e:
        D.inflate_parallel_multi(bytes(bad), chunk_bytes=1024)
    assert e.value.code == -E["E_CRC"]
