"""One foreign stream decoded in one pass on the device (dmx_inflate_parallel_plan_async,
dmx_inflate_parallel_decode_async, inflate_parallel): the device plan against the host plan, the
decode against the data, the two-call idiom, the statuses, 200 single-bit flips against zlib, a
captured graph.  The bounded cases come first in file order; the serial-route and zeros cases run
behind them, and only when all of those passed.

Comparing plans: the record is compared field for field, the live chunks too.  Where the plan has a
status its last chunk is the one whose decode failed: its bit and out_off are compared, its end_bit
and out_len are where that decode stopped, which the header leaves unspecified (the host checks the
end of the input per token, the device per run of tokens)."""
import functools
import zlib

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
import inflate_parallel_dev_inputs as P
import inflate_parallel_inputs as I
import refill_inputs as R

pytestmark = pytest.mark.gpu

E = D.E
SZ, RANGE, HUFDIS = -E["E_SZ"], -E["E_RANGE"], -E["E_HUFDIS"]
FMT = {"auto": 0, "zlib": 1, "gzip": 2, "raw": 3}
CANARY = 0xA5
GUARD = 64

_bounded = {}   # bounded case -> passed; the unbounded cases run when every one of them did


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


# ---- inputs ------------------------------------------------------------------------------------
def inputs():
    """{name: (stream, fmt, data or None, chunk_bytes)}"""
    d = {}
    for name, z, fmt, data in I.round_trip_inputs():
        d[name + "@4096"] = (z, "raw" if fmt == "raw" else "auto", data, 4096)
    name, z, fmt, data = I.round_trip_inputs()[3]
    assert name == "l6-zlib"
    d["l6-zlib@1024"] = (z, "auto", data, 1024)
    d["l6-zlib@65536"] = (z, "auto", data, 65536)
    d["edge@1024"] = (I.window_edge_stream()[0], "auto", I.window_edge_stream()[1], 1024)
    d["run@1024"] = (P.run_stream()[0], "auto", P.run_stream()[1], 1024)
    d["stored@1024"] = (I.stored_only_stream()[0], "auto", I.stored_only_stream()[1], 1024)
    d["fixed@1024"] = (I.fixed_only_stream()[0], "auto", I.fixed_only_stream()[1], 1024)
    d["false3000@1024"] = (I.false_candidate_stream(3000)[0], "auto", I.false_candidate_stream(3000)[1], 1024)
    d["false30000@1024"] = (I.false_candidate_stream(30000)[0], "auto", None, 1024)   # gave_up
    z = I.round_trip_inputs()[3][1]
    for tag, bad in (("empty", b""), ("one-byte", b"\x78"), ("cmpmt", b"\x77\x9c" + z[2:]), ("cut-1000", z[:1000]),
                     ("cut-trailer", z[:-2]), ("junk-behind", z + b"junk")):
        d[tag + "@1024"] = (bad, "auto", None, 1024)
    return d


NAMES = ([n + "@4096" for n in ("l1-zlib", "l1-gzip", "l1-raw", "l6-zlib", "l6-gzip", "l6-raw", "l9-zlib", "l9-gzip", "l9-raw",
                                "l6-zlib-sync3000")] +
         ["l6-zlib@1024", "l6-zlib@65536", "edge@1024", "run@1024", "stored@1024", "fixed@1024", "false3000@1024",
          "false30000@1024", "empty@1024", "one-byte@1024", "cmpmt@1024", "cut-1000@1024", "cut-trailer@1024",
          "junk-behind@1024"])
GOOD = [n for n in NAMES if n.split("@")[0] not in ("false30000", "empty", "one-byte", "cmpmt", "cut-1000", "cut-trailer",
                                                    "junk-behind")]
_inputs = {}


def inp(name):
    if not _inputs:
        _inputs.update(inputs())
        assert sorted(_inputs) == sorted(NAMES)
    return _inputs[name]


def on_device(z, shift=0):
    """z in device memory, `shift` bytes above the start of its allocation"""
    buf = torch.zeros(len(z) + shift + 8, dtype=torch.uint8, device="cuda")
    if z:
        buf[shift:shift + len(z)] = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    return buf[shift:shift + len(z)]


def record(t):
    return D.ParStatus.from_buffer_copy(t.cpu().numpy().tobytes()[:56])


def fields(rec):
    return {f: int(getattr(rec, f)) for f, _ in D.ParStatus._fields_}


def plan_dev(zt, fmt, chunk):
    L = D.lib()
    pb = L.dmx_inflate_parallel_plan_work(zt.numel(), chunk)
    assert pb and pb % 256 == 0
    plan = torch.full((pb,), 0x5A, dtype=torch.uint8, device="cuda")
    assert D.inflate_parallel_plan_async(zt, FMT[fmt], chunk, plan) == 0
    rec = record(plan[:56])
    chunks = plan[256:256 + 32 * rec.nlive].cpu().numpy().view(D.PCHUNK_DTYPE) if rec.nlive <= rec.nchunks else None
    return plan, rec, chunks


def same_plan(z, fmt, chunk, rec, chunks, what):
    hc, hi = D.inflate_parallel_plan_host(z, fmt=fmt, chunk_bytes=chunk)
    assert fields(rec) == hi, (what, fields(rec), hi)
    assert chunks is not None and len(chunks) == len(hc), what
    n = len(hc) - (1 if hi["status"] else 0)
    assert chunks[:n].tobytes() == hc[:n].tobytes(), what
    if hi["status"] and len(hc):
        assert (int(chunks["bit"][-1]), int(chunks["out_off"][-1])) == (int(hc["bit"][-1]), int(hc["out_off"][-1])), what
    return hi


def decode_dev(zt, plan, max_live, out_cap, work_bytes, verify=True):
    big = torch.full((out_cap + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    work = torch.empty(max(work_bytes, 256), dtype=torch.uint8, device="cuda")
    st = torch.full((7,), -1, dtype=torch.int64, device="cuda")
    r = D.inflate_parallel_decode_async(zt, plan, max_live, big[GUARD:GUARD + out_cap] if out_cap else None, out_cap,
                                        work[:work_bytes], verify, st)
    assert r == 0
    return record(st), big.cpu().numpy()


def untouched(big, lo=0):
    """every byte of the guarded buffer from output position lo on still holds the canary"""
    return bool((big[:GUARD] == CANARY).all() and (big[GUARD + lo:] == CANARY).all())


# ---- bounded: the plan ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@bounded
def test_device_plan_equals_host_plan(name):
    z, fmt, data, chunk = inp(name)
    _, rec, chunks = plan_dev(on_device(z), fmt, chunk)
    hi = same_plan(z, fmt, chunk, rec, chunks, name)
    tag = name.split("@")[0]
    if name in GOOD:
        assert hi["status"] == 0 and hi["out_len"] == len(data)
        if tag[0] == "l":   # the round trips: the numbers the decode's cases stand on, from the host plan
            assert hi["nlive"] >= 8
            if "sync" not in tag:   # (a sync flush every 3 000 bytes: 155 chunks of 9 000 to 12 000 bytes)
                assert int(np.max(D.inflate_parallel_plan_host(z, fmt=fmt, chunk_bytes=chunk)[0]["out_len"])) > 32768
        if tag in ("stored", "fixed"):
            assert hi["nlive"] == 1
        if tag == "false3000":
            assert hi["ndead"] >= 1
    elif tag == "false30000":
        assert (hi["status"], hi["gave_up"]) == (RANGE, 1)
    elif tag == "junk-behind":
        assert hi["status"] == 0 and hi["in_used"] == len(z) - 4
    else:
        assert hi["status"] == -E[{"empty": "E_ZHEAD", "one-byte": "E_ZHEAD", "cmpmt": "E_ZCMPMT", "cut-1000": "E_LEN",
                                   "cut-trailer": "E_ZADL32"}[tag]]


# ---- bounded: the decode --------------------------------------------------------------------------
def _check_decode(name, z, fmt, data, chunk, shift=0, verify=True, slack=0):
    zt = on_device(z, shift)
    plan, rec, chunks = plan_dev(zt, fmt, chunk)
    hi = same_plan(z, fmt, chunk, rec, chunks, name)
    assert hi["status"] == 0
    cap = hi["out_len"] + slack
    got, big = decode_dev(zt, plan, hi["nlive"] + (3 if slack else 0), cap,
                          D.lib().dmx_inflate_parallel_work(cap, hi["nlive"] + 3) if slack else hi["work_len"], verify)
    assert fields(got) == hi, (name, fields(got), hi)
    assert got.format == {"auto": 2 if z[:2] == b"\x1f\x8b" else 1, "raw": 3}[fmt]
    assert big[GUARD:GUARD + len(data)].tobytes() == data, name
    assert untouched(big, len(data)), name   # nothing behind out_len, nothing behind out_cap


@pytest.mark.parametrize("name", GOOD)
@bounded
def test_decode(name):
    z, fmt, data, chunk = inp(name)
    _check_decode(name, z, fmt, data, chunk)


@pytest.mark.parametrize("name", ["l6-gzip@4096", "run@1024", "edge@1024"])
@pytest.mark.parametrize("shift", [1, 3])
@bounded
def test_decode_unaligned_input_and_larger_output(name, shift):
    z, fmt, data, chunk = inp(name)
    _check_decode(name, z, fmt, data, chunk, shift=shift, slack=1000 + shift)


@pytest.mark.parametrize("name", ["l6-zlib@4096", "l9-gzip@4096", "l1-raw@4096", "run@1024"])
@bounded
def test_decode_without_verify(name):
    z, fmt, data, chunk = inp(name)
    _check_decode(name, z, fmt, data, chunk, verify=False)
    if fmt != "raw":   # a wrong check value passes, the bytes are the same
        zb = bytearray(z)
        zb[-1 if z[:2] != b"\x1f\x8b" else -5] ^= 1
        zt = on_device(bytes(zb))
        plan, rec, _ = plan_dev(zt, fmt, chunk)
        got, big = decode_dev(zt, plan, rec.nlive, rec.out_len, rec.work_len, verify=False)
        assert got.status == 0 and big[GUARD:GUARD + len(data)].tobytes() == data


# ---- bounded: the two-call idiom ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["l6-zlib@4096", "run@1024"])
@bounded
def test_capacities_too_small(name):
    z, fmt, data, chunk = inp(name)
    zt = on_device(z)
    plan, rec, _ = plan_dev(zt, fmt, chunk)
    assert rec.status == 0 and rec.nlive > 1
    for what, (ml, cap, wb) in (("out_cap", (rec.nlive, rec.out_len - 1, rec.work_len)),
                                ("max_live", (rec.nlive - 1, rec.out_len, rec.work_len)),
                                ("work_bytes", (rec.nlive, rec.out_len, rec.work_len - 256))):
        got, big = decode_dev(zt, plan, ml, cap, wb)
        assert got.status == SZ, (what, got.status)
        assert (got.nlive, got.out_len, got.work_len) == (rec.nlive, rec.out_len, rec.work_len), what
        assert untouched(big), what
    got, big = decode_dev(zt, plan, rec.nlive, rec.out_len, rec.work_len)   # and the exact numbers pass
    assert got.status == 0 and big[GUARD:GUARD + len(data)].tobytes() == data


@bounded
def test_a_plan_that_gave_up():
    z, fmt, _, chunk = inp("false30000@1024")
    zt = on_device(z)
    plan, rec, _ = plan_dev(zt, fmt, chunk)
    assert (rec.status, rec.gave_up) == (RANGE, 1)
    got, big = decode_dev(zt, plan, rec.nchunks, 200_000, D.lib().dmx_inflate_parallel_work(200_000, rec.nchunks))
    assert fields(got) == fields(rec) and untouched(big)
    for tag in ("cut-1000@1024", "empty@1024"):   # any other plan status too
        z, fmt, _, chunk = inp(tag)
        zt = on_device(z)
        plan, rec, _ = plan_dev(zt, fmt, chunk)
        got, big = decode_dev(zt, plan, 100, 100_000, D.lib().dmx_inflate_parallel_work(100_000, 100))
        assert rec.status != 0 and fields(got) == fields(rec) and untouched(big), tag


# ---- bounded: statuses ------------------------------------------------------------------------------
def _status_of(z, fmt="auto", chunk=4096):
    zt = on_device(z)
    plan, rec, chunks = plan_dev(zt, fmt, chunk)
    same_plan(z, fmt, chunk, rec, chunks, "status")
    if rec.status:
        return rec.status, rec, None
    got, big = decode_dev(zt, plan, rec.nlive, rec.out_len, rec.work_len)
    assert untouched(big, rec.out_len)
    if got.status:
        assert (got.out_len, got.in_used, got.check, got.work_len) == (0, 0, 0, 0)
    return got.status, rec, big


@bounded
def test_trailer_statuses():
    z = bytearray(I.round_trip_inputs()[3][1])
    z[-2] ^= 0x10
    assert _status_of(bytes(z))[0] == -E["E_ZADL32"]
    gz = I.round_trip_inputs()[4][1]
    assert gz[:2] == b"\x1f\x8b"
    z = bytearray(gz)
    z[-6] ^= 1   # CRC-32
    assert _status_of(bytes(z))[0] == -E["E_CRC"]
    z = bytearray(gz)
    z[-3] ^= 1   # ISIZE
    assert _status_of(bytes(z))[0] == -E["E_LEN"]
    z[-6] ^= 1   # both: the CRC is checked first
    assert _status_of(bytes(z))[0] == -E["E_CRC"]
    assert _status_of(gz)[0] == 0


@bounded
def test_a_distance_before_the_first_byte():
    for name, z, off in P.too_far_streams():
        status, rec, _ = _status_of(z, chunk=1024)
        assert rec.status == 0 and status == HUFDIS, (name, status)
        with pytest.raises(D.DeflateError) as e:
            D.deflate_decompress(z)
        assert e.value.code == HUFDIS, name
        assert (rec.nlive > 1) == (name == "later-chunk")


@bounded
def test_single_bit_flips():
    z, data, flips = I.flip_stream()
    assert len(flips) == 200
    accepted = wanted = 0
    for k, f in enumerate([z] + flips):   # (case 0: the stream itself, the one zlib accepts -- its Adler-32 refuses all 200 flips)
        try:
            want = zlib.decompress(f)
        except zlib.error:
            want = None
        wanted += want is not None
        zt = on_device(f)
        plan, rec, chunks = plan_dev(zt, "auto", 1024)
        hi = same_plan(f, "auto", 1024, rec, chunks, k)
        cap = len(data) + 500
        got, big = decode_dev(zt, plan, rec.nchunks, cap, D.lib().dmx_inflate_parallel_work(cap, rec.nchunks))
        if hi["status"] == 0 and hi["out_len"] > cap:   # (a flip that makes the stream longer than the room given)
            assert want is None or len(want) > cap
            assert got.status == SZ and untouched(big), k
            continue
        if hi["status"]:
            assert got.status == hi["status"] and untouched(big), (k, got.status, hi)
            assert want is None, k
        elif want is None:
            assert got.status != 0, k
        else:
            assert got.status == 0 and got.out_len == len(want) and big[GUARD:GUARD + len(want)].tobytes() == want, k
            accepted += 1
        assert untouched(big, cap), k   # never a byte behind out_cap
    assert accepted == wanted >= 1


# ---- bounded: in a graph ----------------------------------------------------------------------------
@bounded
def test_plan_and_decode_in_a_graph():
    """plan + decode captured once with capacities, replayed on two different streams of one length
    copied into the same tensor, on a corrupt one, and on the first again"""
    t = I.text()
    a, b = t[:300_000], t[310_000:590_000]
    za, zb = I.deflate(a, 6, 15), I.deflate(b, 9, 15)
    n = max(len(za), len(zb)) + 16
    za, zb = za + bytes(n - len(za)), zb + bytes(n - len(zb))   # bytes behind the trailer are ignored
    bad = bytearray(za)
    bad[len(I.deflate(a, 6, 15)) - 1] ^= 1   # the Adler-32
    chunk, cap = 4096, 300_000 + 100
    L = D.lib()
    nc = -(-n // chunk)
    zt = torch.zeros(n, dtype=torch.uint8, device="cuda")
    plan = torch.zeros(L.dmx_inflate_parallel_plan_work(n, chunk), dtype=torch.uint8, device="cuda")
    work = torch.zeros(L.dmx_inflate_parallel_work(cap, nc), dtype=torch.uint8, device="cuda")
    big = torch.zeros(cap + 2 * GUARD, dtype=torch.uint8, device="cuda")
    st = torch.zeros(7, dtype=torch.int64, device="cuda")

    def enqueue():
        r = D.inflate_parallel_plan_async(zt, 0, chunk, plan)
        return r or D.inflate_parallel_decode_async(zt, plan, nc, big[GUARD:GUARD + cap], cap, work, True, st)

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
    for z, data, want in ((zb, b, 0), (za, a, 0), (bytes(bad), None, -E["E_ZADL32"]), (zb, b, 0), (za, a, 0)):
        zt.copy_(torch.frombuffer(bytearray(z), dtype=torch.uint8))
        big.fill_(CANARY)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = record(st)
        assert got.status == want, (got.status, want)
        h = big.cpu().numpy()
        if data is not None:
            assert got.out_len == len(data) and h[GUARD:GUARD + len(data)].tobytes() == data
            assert untouched(h, len(data))
        assert untouched(h, cap)


# ---- the Python route -----------------------------------------------------------------------------
@bounded
def test_inflate_parallel_takes_the_parallel_route():
    for name in ("l6-zlib@4096", "l6-gzip@4096", "l9-raw@4096", "run@1024"):
        z, fmt, data, chunk = inp(name)
        info = {}
        out = D.inflate_parallel(on_device(z), fmt=fmt, chunk_bytes=chunk, info=info)
        assert info["route"] == "parallel" and info["status"] == 0 and info["nlive"] > 1, (name, info)
        assert out.cpu().numpy().tobytes() == data, name
    z, fmt, data, _ = inp("l6-zlib@4096")
    info = {}
    assert D.inflate_parallel(z, info=info).cpu().numpy().tobytes() == data   # bytes, the default cut
    assert info["route"] == "parallel"
    bad = bytearray(z)
    bad[-1] ^= 1
    with pytest.raises(D.DeflateError) as e:
        D.inflate_parallel(bytes(bad), chunk_bytes=4096)
    assert e.value.code == -E["E_ZADL32"]
    with pytest.raises(D.DeflateError) as e:
        D.inflate_parallel(z[:1000], chunk_bytes=1024)
    assert e.value.code == -E["E_LEN"]
    for name in ("stored@1024", "fixed@1024"):   # one chunk: nothing to parallelise
        z, fmt, data, chunk = inp(name)
        info = {}
        out = D.inflate_parallel(z, chunk_bytes=chunk, info=info)
        assert info["route"] == "serial" and info["nlive"] == 1 and out.cpu().numpy().tobytes() == data, name


# ---- unbounded: behind the bounded cases, and only when they all passed ---------------------------
def test_gave_up_takes_the_serial_route():
    need_bounded()
    z, data = I.false_candidate_stream(30000)
    info = {}
    out = D.inflate_parallel(z, chunk_bytes=1024, info=info)
    assert (info["route"], info["status"], info["gave_up"]) == ("serial", RANGE, 1)
    assert out.cpu().numpy().tobytes() == data


@pytest.mark.parametrize("name", ["zeros-5m", "zeros-16m"])
def test_zeros_take_the_serial_route(name):
    need_bounded()
    i = {x.name: x for x in R.zlib_inputs()}[name]
    _, hi = D.inflate_parallel_plan_host(i.z)   # blocks above 4 MiB: the plan gives up
    assert (hi["status"], hi["gave_up"]) == (RANGE, 1)
    info = {}
    out = D.inflate_parallel(i.z, info=info)
    assert (info["route"], info["status"], info["gave_up"]) == ("serial", RANGE, 1)
    assert out.numel() == len(i.data) and int(out.max().item()) == i.data[0] and int(out.min().item()) == i.data[0]


def test_the_largest_single_chunk():
    """4 MiB of zeros at level 6: one chunk of exactly DMX_PF_MAX_CHUNK_OUT, through the async pair --
    the largest single chunk the cell decoder and the tail kernel may see"""
    need_bounded()
    n = 4 << 20
    z = zlib.compress(bytes(n), 6)
    hc, hi = D.inflate_parallel_plan_host(z, chunk_bytes=65536)
    assert (hi["status"], hi["nlive"], int(hc["out_len"][0])) == (0, 1, n)
    zt = on_device(z)
    plan, rec, chunks = plan_dev(zt, "auto", 65536)
    same_plan(z, "auto", 65536, rec, chunks, "4 MiB")
    got, big = decode_dev(zt, plan, 1, n, rec.work_len)
    assert fields(got) == hi
    assert untouched(big, n) and not big[GUARD:GUARD + n].any()
