"""ZIP archives on the MI355X: the device index (dmx_zip_index_async, zip_index_gpu) against the host
walk dmx_zip_index_host -- record and entries byte for byte, on sound, corrupt and truncated
archives, at every alignment -- and the decode of selections of entries (dmx_zip_read_async,
zip_read, unzip) against CPython's zipfile: bytes, offsets, results, the summary, guard bytes
around the output, per-entry faults that leave the neighbours alone, and both calls in one graph.
No test provokes a device fault: corrupt inputs end in statuses, which tests/c/zip_model.cpp
establishes on the host first."""
import ctypes
import functools
import io
import zipfile

import numpy as np
import pytest
import torch

import deflate_compression_amd as D
import zip_inputs as Z

pytestmark = pytest.mark.gpu

E = D.E
SZ, RANGE, CRC, LEN = -E["E_SZ"], -E["E_RANGE"], -E["E_CRC"], -E["E_LEN"]
GUARD = 64
ZCAP = 1 << 20
CAPMAX = 2048


class Bufs:
    """device buffers every index case shares: the archive (with room to shift it), the entries, the
    record, the work buffer"""

    def __init__(self):
        L = D.lib()
        self.z = torch.zeros(ZCAP + 64, dtype=torch.uint8, device="cuda")
        self.entries = torch.zeros((CAPMAX + 1) * 64, dtype=torch.uint8, device="cuda")
        self.st = torch.zeros(40, dtype=torch.uint8, device="cuda")
        self.max_cand = ZCAP // 46 + 8
        self.work = torch.zeros(int(L.dmx_zip_index_work(ZCAP, self.max_cand)), dtype=torch.uint8, device="cuda")
        assert self.work.data_ptr() % 256 == 0 and self.z.data_ptr() % 16 == 0


@functools.lru_cache(maxsize=None)
def _bufs() -> Bufs:
    return Bufs()


def _upload(z: bytes, head: int = 0):
    B = _bufs()
    assert len(z) + head <= B.z.numel()
    if z:
        B.z[head:head + len(z)].copy_(torch.frombuffer(bytearray(z), dtype=torch.uint8))
    return B.z[head:head + len(z)]


def _gpu_index(z: bytes, head: int = 0, cap: int = CAPMAX, work_bytes: int | None = None):
    """(record bytes, entry bytes of all CAPMAX + 1 slots) of dmx_zip_index_async"""
    B = _bufs()
    zt = _upload(z, head)
    B.entries.fill_(0xEE)
    B.st.fill_(0xEE)
    work = B.work if work_bytes is None else B.work[:work_bytes]
    assert D.zip_index_async(zt, B.entries, cap, work, B.st) == 0
    torch.cuda.synchronize()
    return B.st.cpu().numpy().tobytes(), B.entries.cpu().numpy().tobytes()


def _host_index(z: bytes, cap: int = CAPMAX):
    L = D.lib()
    st = D.ZipStatus()
    ent = np.full((CAPMAX + 1) * 64, 0xEE, dtype=np.uint8)
    buf = ctypes.create_string_buffer(z, len(z) or 1)
    assert L.dmx_zip_index_host(buf, len(z), ctypes.c_void_p(ent.ctypes.data), cap, ctypes.byref(st)) == 0
    return bytes(st), ent.tobytes()


def _same(z: bytes, head: int = 0, cap: int = CAPMAX, what=""):
    g, h = _gpu_index(z, head, cap), _host_index(z, cap)
    assert g[0] == h[0], (what, head, D.ZipStatus.from_buffer_copy(g[0]).status, D.ZipStatus.from_buffer_copy(h[0]).status)
    assert g[1] == h[1], (what, head)   # (also: nothing behind the entries that were due)


def _all_inputs() -> dict:
    d = dict(Z.cases())
    d["comment_sig"] = Z.comment_with_end_signature()
    for k, v in Z.corrupt_cases().items():
        d["corrupt_" + k] = v[0]
    return d


@pytest.mark.parametrize("name", sorted(_all_inputs()))
def test_index_equals_host(name):
    z = _all_inputs()[name]
    for head in (0, 5):
        _same(z, head, what=name)


def test_index_alignments_and_prefixes():
    z = Z.cases()["seams_600"]
    for head in range(16):
        _same(z, head, what="seams")
    ents = Z.small_entries(600, 30)
    for pre in range(1, 16):
        _same(Z.craft(ents, prefix=b"p" * pre), 0, what=f"prefix {pre}")


def test_index_truncations():
    z = Z.craft(Z.small_entries(4) + [Z.Ent("s", b"stored", 0)], comment=b"hi")
    for n in range(len(z)):
        _same(z[:n], n & 15, what=f"cut {n}")
    z = Z.craft(Z.small_entries(3), zip64=True, prefix=b"xy")
    for n in range(len(z) - 120, len(z)):
        _same(z[:n], 0, what=f"cut64 {n}")


def test_index_small_buffers():
    z = Z.cases()["count_65"]
    _same(z, 3, cap=10, what="cap 10")        # -E_SZ: the first 10 entries, the full counts
    _same(z, 0, cap=0, what="cap 0")
    need = int(D.lib().dmx_zip_index_work(len(z), 1))
    rec, ent = _gpu_index(z, 0, work_bytes=need)
    st = D.ZipStatus.from_buffer_copy(rec)
    assert (st.status, st.nentries, st.out_len, st.ncand) == (SZ, 0, 0, 65)
    assert ent == b"\xee" * len(ent)
    # zip_index_gpu takes the second pass with the number the first reports
    zt = _upload(z, 7)
    ix = D.zip_index_gpu(zt, _max_cand=1)
    ref = D.zip_index(z)
    assert ix.host.tobytes() == ref.host.tobytes() and bytes(ix.status) == bytes(ref.status)
    with pytest.raises(D.DeflateError) as ei:
        D.zip_index_gpu(zt, cap=10)
    assert ei.value.code == SZ
    assert D.zip_index_gpu(zt).names == ref.names


# ---- the decode ----

def _read(z: bytes, sel=None, verify=True, entries=None, head=0, out_bytes=None):
    """dmx_zip_read_async with guard bytes around the output: (out bytes, offsets, results, record)"""
    L = D.lib()
    zt = _upload(z, head)
    if entries is None:
        entries = Z.entry_array(z)[1]
    ne = len(entries)
    et = torch.from_numpy(np.ascontiguousarray(entries).view(np.uint8).reshape(-1).copy() if ne else np.zeros(64, np.uint8)).cuda()
    if sel is None:
        n, st_sel = ne, None
        pick = list(range(ne))
    else:
        pick = list(sel)
        n = len(pick)
        st_sel = torch.from_numpy(np.array(pick + [0], dtype=np.uint32).view(np.int32)).cuda()
    total = sum(int(entries[j]["usize"]) for j in pick if j < ne and int(entries[j]["status"]) == 0)
    ob = total if out_bytes is None else out_bytes
    out = torch.full((GUARD + ob + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    res = torch.full((max(n, 1) * 4,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(int(L.dmx_zip_read_work(n)), dtype=torch.uint8, device="cuda")
    r = D.zip_read_async(zt, et, ne, st_sel, n, D.DMX_ZIP_VERIFY if verify else 0, out[GUARD:GUARD + ob] if ob else None, ob,
                         offsets, res, work, st)
    assert r == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:GUARD] == 0xA5).all() and (o[GUARD + ob:] == 0xA5).all()
    results = res.view(max(n, 1), 4)[:n].cpu().numpy().view(np.uint8).reshape(-1).view(D.BRESULT_DTYPE)
    rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
    return o[GUARD:GUARD + ob].tobytes(), offsets.cpu().numpy(), results, rec


def _check_against_zipfile(z, pick, data, offsets, results, rec, verify=True):
    ref = Z.zipfile_entries(z)
    run = 0
    for k, j in enumerate(pick):
        info, _, want = ref[j]
        assert int(offsets[k]) == run
        assert data[run:run + len(want)] == want, (k, j, info.filename)
        r = results[k]
        assert (int(r["status"]), int(r["format"]), int(r["out_len"]), int(r["check"])) == \
            (0, info.compress_type, len(want), info.CRC), (k, j)
        assert int(r["in_used"]) <= info.compress_size and (info.compress_type or int(r["in_used"]) == len(want))
        run += len(want)
    assert int(offsets[len(pick)]) == run == len(data)
    assert (rec.nfailed, rec.first_bad, rec.total_out) == (0, 0xFFFFFFFF, run)


READ_CASES = ("count_0", "count_1", "count_3", "count_65", "count_257", "count_1025", "seams_600", "lookalikes", "nested_last",
              "payloads", "zip64_all", "zip64_mix", "data_descriptors", "local_extra", "zip64_prefix_comment",
              "prefix_70", "zipfile_written")


@pytest.mark.parametrize("name", READ_CASES)
def test_read_all_entries(name):
    z = Z.cases()[name]
    n = len(Z.zipfile_entries(z))
    for head, verify in ((0, True), (9, False)):
        data, offsets, results, rec = _read(z, head=head, verify=verify)
        _check_against_zipfile(z, list(range(n)), data, offsets, results, rec)


def test_stored_copy_every_alignment():
    """source and destination of the copy kernel at all 16 distances modulo 16 (equal among them: the
    unshifted path), entries that end inside a span, span the seam between two and fill several"""
    span = ctypes.c_uint32(0)
    D.lib().dmx_zip_read_geometry(ctypes.byref(span))
    s = span.value
    sizes = (s - 7, 15, 1, 2 * s + 33, 16, 0, 17, s // 2)
    z = Z.craft([Z.Ent(f"s{i}", Z.noise(n, 60 + i), 0) for i, n in enumerate(sizes)])
    for head in range(16):
        data, offsets, results, rec = _read(z, head=head)
        _check_against_zipfile(z, list(range(len(sizes))), data, offsets, results, rec)
    data, offsets, results, rec = _read(z, sel=[3, 0, 3], head=4, verify=False)
    _check_against_zipfile(z, [3, 0, 3], data, offsets, results, rec)


def test_selections():
    z = Z.cases()["payloads"]
    n = len(Z.payload_entries())
    for pick in (list(range(n))[::-1], [7, 2, 5], [7, 7, 0, 7, 4, 4], [1], []):
        data, offsets, results, rec = _read(z, sel=pick)
        _check_against_zipfile(z, pick, data, offsets, results, rec)
    # by name, through zip_read
    zt = _upload(z, 2)
    ix = D.zip_index_gpu(zt)
    out, offsets, results = D.zip_read(zt, ix, which=["noise_100k_stored", 4, "one_byte", "text_70k"])
    ref = {i.filename: d for i, _, d in Z.zipfile_entries(z)}
    want = ref["noise_100k_stored"] + ref["three_blocks"] + ref["one_byte"] + ref["text_70k"]
    assert out.cpu().numpy().tobytes() == want and int(offsets[-1]) == len(want) and (results["status"] == 0).all()
    out, offsets, results = D.zip_read(zt, ix, which=[])
    assert out.numel() == 0 and offsets.cpu().tolist() == [0] and len(results) == 0
    out, offsets, results = D.zip_read(zt)   # indexed here
    assert out.cpu().numpy().tobytes() == b"".join(d for _, _, d in Z.zipfile_entries(z))


def test_per_entry_faults():
    z = Z.cases()["count_65"]
    _, clean = Z.entry_array(z)
    ref = Z.zipfile_entries(z)
    base = _read(z)
    k = 34   # a deflated entry in the middle
    assert int(clean[k]["method"]) == 8 and int(clean[k]["usize"]) > 1

    def run(mutate, verify=True, sel=None):
        ent = clean.copy()
        mutate(ent)
        return _read(z, sel=sel, verify=verify, entries=ent)

    def neighbours(got, bad, nfailed=1):
        data, offsets, results, rec = got
        for j in range(65):
            if j == bad:
                continue
            want = ref[j][2]
            assert data[int(offsets[j]):int(offsets[j]) + len(want)] == want, j
            assert results[j].tobytes() == base[2][j].tobytes(), j
        assert (rec.nfailed, rec.first_bad) == (nfailed, bad if nfailed else 0xFFFFFFFF)
        assert rec.total_out == sum(int(r["out_len"]) for r in results)

    def flip_crc(e):
        e[k]["crc"] ^= 0x10
    got = run(flip_crc)
    assert int(got[2][k]["status"]) == CRC and int(got[2][k]["out_len"]) == 0
    neighbours(got, k)
    got = run(flip_crc, verify=False)
    assert int(got[2][k]["status"]) == 0 and int(got[2][k]["check"]) == int(clean[k]["crc"]) ^ 0x10
    neighbours(got, k, nfailed=0)

    def longer(e):
        e[k]["usize"] += 1
    got = run(longer)
    assert int(got[2][k]["status"]) == LEN
    neighbours(got, k)

    def shorter(e):
        e[k]["usize"] -= 1
    got = run(shorter)
    assert int(got[2][k]["status"]) == SZ
    neighbours(got, k)

    def cut(e):
        e[k]["csize"] -= 1
    a, c = int(clean[k]["data_off"]), int(clean[k]["csize"])
    _, _, want = D.inflate_batch([z[a:a + c - 1]], fmt="raw", sizes=[int(clean[k]["usize"])], strict=False)
    expect = int(want[0]["status"]) or LEN
    got = run(cut)
    assert int(got[2][k]["status"]) == expect and expect != 0
    neighbours(got, k)

    # a stored entry whose CRC is wrong, and a selector out of range
    s = 33
    assert int(clean[s]["method"]) == 0

    def flip_stored(e):
        e[s]["crc"] ^= 1
    got = run(flip_stored)
    assert int(got[2][s]["status"]) == CRC
    neighbours(got, s)
    pick = list(range(65))
    pick[k] = 65
    data, offsets, results, rec = _read(z, sel=pick)
    assert int(results[k]["status"]) == RANGE and int(offsets[k + 1]) == int(offsets[k])
    assert (rec.nfailed, rec.first_bad) == (1, k)
    for j in range(65):
        if j != k:
            want = ref[j][2]
            assert data[int(offsets[j]):int(offsets[j]) + len(want)] == want


def test_index_statuses_reach_the_results():
    z, _, idx, estat = Z.corrupt_cases()["method_12"]
    data, offsets, results, rec = _read(z)
    ref = Z.zipfile_entries(Z.corrupt_cases()["base"][0])
    assert int(results[idx]["status"]) == estat and int(offsets[idx + 1]) == int(offsets[idx])
    assert (rec.nfailed, rec.first_bad) == (1, idx)
    for j, (info, _, want) in enumerate(ref):
        if j != idx:
            assert data[int(offsets[j]):int(offsets[j + 1])] == want and int(results[j]["status"]) == 0


def test_output_too_small_writes_nothing():
    z = Z.cases()["payloads"]
    total = sum(len(d) for _, _, d in Z.zipfile_entries(z))
    data, offsets, results, rec = _read(z, out_bytes=total - 1)
    assert data == b"\xa5" * (total - 1)
    assert (results["status"] == SZ).all() and int(offsets[-1]) == total
    assert (rec.nfailed, rec.first_bad, rec.total_out) == (len(results), 0, total)


def test_index_and_read_in_a_graph():
    """zip_index_async + zip_read_async captured once and replayed on archives of the same length,
    copied into the same tensor; one of them needs more output than the graph has"""
    L = D.lib()

    def archive(seed, big=False):
        ents = [Z.Ent(f"f{i}", Z.text(500 + 700 * ((i + seed) % 4), seed * 10 + i), 8 if (i + seed) % 3 else 0) for i in range(9)]
        if big:
            ents[4] = Z.Ent("big", Z.text(60000, seed), 8)
        return ents
    size = 60000
    zs = []
    for seed, big in ((1, False), (2, False), (3, True)):
        z0 = Z.craft(archive(seed, big))
        zs.append(Z.craft(archive(seed, big), comment=b"c" * (size - len(z0))))
        assert len(zs[-1]) == size
    cap, ocap = 16, 30000
    zt = torch.zeros(size, dtype=torch.uint8, device="cuda")
    ent = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
    ist = torch.zeros(40, dtype=torch.uint8, device="cuda")
    iwork = torch.zeros(int(L.dmx_zip_index_work(size, 1024)), dtype=torch.uint8, device="cuda")
    out = torch.zeros(GUARD + ocap + GUARD, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(10, dtype=torch.int64, device="cuda")
    res = torch.zeros(9 * 4, dtype=torch.int64, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    rwork = torch.zeros(int(L.dmx_zip_read_work(9)), dtype=torch.uint8, device="cuda")

    def enqueue():
        r = D.zip_index_async(zt, ent, cap, iwork, ist)
        return r or D.zip_read_async(zt, ent, 9, None, 9, D.DMX_ZIP_VERIFY, out[GUARD:GUARD + ocap], ocap, offsets, res, rwork, st)

    zt.copy_(torch.frombuffer(bytearray(zs[0]), dtype=torch.uint8))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # not captured: the kernels are loaded before the capture
        assert enqueue() == 0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r = enqueue()
    assert r == 0
    for z in (zs[1], zs[2], zs[0]):
        zt.copy_(torch.frombuffer(bytearray(z), dtype=torch.uint8))
        out.fill_(0xA5)
        res.fill_(-1)
        st.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ref = Z.zipfile_entries(z)
        total = sum(len(d) for _, _, d in ref)
        o = out.cpu().numpy()
        results = res.cpu().numpy().view(np.uint8).view(D.BRESULT_DTYPE)
        rec = D.BatchStatus.from_buffer_copy(st.cpu().numpy().tobytes())
        irec = D.ZipStatus.from_buffer_copy(ist.cpu().numpy().tobytes())
        assert (irec.status, irec.nentries, irec.out_len) == (0, 9, total)
        assert (o[:GUARD] == 0xA5).all() and (o[GUARD + ocap:] == 0xA5).all()
        if total > ocap:
            assert (o == 0xA5).all()
            assert (results["status"] == SZ).all() and (rec.nfailed, rec.first_bad, rec.total_out) == (9, 0, total)
        else:
            _check_against_zipfile(z, list(range(9)), o[GUARD:GUARD + total].tobytes(), offsets.cpu().numpy(), results, rec)


def test_unzip():
    z = Z.cases()["zipfile_written"]
    with zipfile.ZipFile(io.BytesIO(z)) as zf:
        want = {i.filename: zf.read(i) for i in zf.infolist()}
    assert "dir/" in want and D.unzip(z) == want
    assert D.unzip(Z.cases()["count_0"]) == {}
    with pytest.raises(D.DeflateError):
        D.unzip(Z.corrupt_cases()["method_12"][0])
