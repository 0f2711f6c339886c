"""The inputs of tests/refill_inputs.py do what they claim, on the CPU: zlib and the host decoder
agree on every stream's bytes, and the model of the device reader's two refill places
(refill_inputs.refill_model) finds the stretches of mid-token refills that
tests/test_gpu_refill.py needs -- long in every "starving" input, absent in every control and in
the suite's text streams.

The bounds.  The reader's two stream segments hold 128 words from wb on; a mid-token refill that
does not rotate reads wrongly once wi - wb reaches 128, and after a rotation wi - wb is at most
64, so a run of 128 such refills always reads a word wrongly and a run of 64 may.  Starving
inputs have runs of at least 256 (twice that: 64 for the phase the stretch starts at, the rest
margin); controls at most 2; text at most 8.  zlib's streams of 768 KiB and 1 MiB of zeros are one
block of 190 and 254 words: kept apart ("short"), at least 128."""
import zlib

import pytest

import deflate_compression_amd as D
import inflate_parallel_inputs as I
import refill_inputs as R

WBITS = {"zlib": 15, "gzip": 31, "raw": -15}


@pytest.fixture(scope="module")
def inputs():
    return R.crafted_inputs() + R.zlib_inputs()


def test_names_and_kinds(inputs):
    names = [i.name for i in inputs]
    assert len(set(names)) == len(names)
    for T in (2, 4, 8, 16):   # every power-of-two geometry in both alignments
        assert any(i.T == T and i.kind == "starving" for i in inputs), T
        assert any(i.T == T and i.kind == "control" for i in inputs), T
    assert {i.T for i in inputs if i.kind == "control"} >= {3, 6}
    assert {i.fmt for i in inputs} == {"zlib", "gzip", "raw"}
    # each block is a few thousand tokens and at most about 1.3 MB of output
    assert all(len(i.data) < 1_400_000 for i in R.crafted_inputs())
    assert max(len(i.z) for i in inputs) < 50_000


def test_zlib_and_host_decoder_agree(inputs):
    for i in inputs:
        assert zlib.decompress(i.z, WBITS[i.fmt]) == i.data, i.name
        if i.fmt == "raw":
            got, used = D.inflate_dict_host(i.z, None, "raw")
            assert got == i.data and used == len(i.z), i.name
        else:
            assert D.deflate_decompress(i.z) == i.data, i.name


def test_tokens_have_one_size(inputs):
    """the crafted block of every geometry: NTOK matches of exactly T bits, one behind the other"""
    for i in R.crafted_inputs():
        blocks = [b for b in R.parse(i.z, 16) if b[2] and len(b[2]) > R.NTOK]
        assert len(blocks) == 1, i.name
        m = [(s, a, e) for s, a, e in blocks[0][2] if a != e]
        assert len(m) == R.NTOK and {e - s for s, a, e in m} == {i.T}, i.name
        assert all(m[k][2] == m[k + 1][0] for k in range(len(m) - 1)), i.name
        assert len({a - s for s, a, e in m}) == 1, i.name


def test_model_runs(inputs):
    for i in inputs:
        r = R.model_of(i)
        print(i.name, i.kind, len(i.z), len(i.data), r)
        if i.kind == "starving":
            assert r.run >= 256 and r.span >= 256, (i.name, r)
        elif i.kind == "short":
            assert r.run >= 128 and r.span >= 128, (i.name, r)
        else:
            assert r.run <= 2 and r.span <= 64, (i.name, r)


def test_model_runs_at_every_alignment(inputs):
    """a stream that does not begin on a 4-byte boundary (a batch packs them back to back): tokens
    of up to 8 bits starve the same; 16-bit tokens only where the shift is a multiple of 16 bits"""
    for i in inputs:
        for lo in (1, 2, 3):
            r = R.model_of(i, lo)
            if i.kind == "starving" and (i.T <= 8 or lo == 2):
                assert r.run >= 256, (i.name, lo, r)
            elif i.kind == "short":
                assert r.run >= 128, (i.name, lo, r)
            elif i.kind == "control" and (i.T <= 8 or lo == 2):
                assert r.run <= 2, (i.name, lo, r)


def test_model_with_both_refills_rotating(inputs):
    """the rule of the fix: no mid-token refill reads beyond the first word of vnxt"""
    for i in inputs:
        r = R.model_of(i, fixed=True)
        assert r.span <= 64, (i.name, r)
    tail = {i.name: R.model_of(i, fixed=True).tail_mid for i in inputs}
    # the stretch reaches into the last 192 words, where the run hands the refill to its caller
    assert tail["t2-zero-at-end"] >= 64 and tail["t4-at-end"] >= 64, tail
    assert tail["zeros-1m"] >= 64 and tail["t2-zero-starving"] == 0, tail


def test_far_stream_reaches_the_window_edge():
    i = next(x for x in R.crafted_inputs() if x.name == "t16-far-starving")
    assert i.data[32768 + 258:32768 + 2 * 258] != i.data[32768:32768 + 258]
    d = [dist for _, dist in R.far_matches()]
    assert len(d) == R.NTOK and min(d) >= 16385 and max(d) <= 32768
    # every 50th match is exactly the window back; the others are drawn from all 16 384 distances
    assert d.count(32768) >= R.NTOK // 50 and min(d) < 16385 + 64, (min(d), max(d))


def test_dictionary_streams():
    zdict, streams = R.dict_inputs()
    for name, raw, data in streams:
        d = zlib.decompressobj(-15, zdict=zdict)
        assert d.decompress(raw) == data and d.eof, name
        got, used = D.inflate_dict_host(raw, zdict, "raw")
        assert got == data and used == len(raw), name
        assert R.refill_model(raw).run >= 256, name
        # without the dictionary the first match reaches before the output
        with pytest.raises(zlib.error):
            zlib.decompress(raw, -15)


def test_text_streams_never_starve():
    for name, z, fmt, data in I.round_trip_inputs():
        r = R.refill_model(z, R.body_bit(z, fmt))
        assert r.run <= 8 and r.span < 128, (name, r)
    z, t = R.text_stream()
    assert zlib.decompress(z) == t and R.refill_model(z, 16).run <= 8


def test_cut_streams_end_early_on_the_host():
    """every cut stream is -E_LEN to the host decoder, with and without a dictionary, and zlib
    wants more input; what the zeros behind the cut spell is what the case's name says"""
    cuts = R.cut_inputs()
    assert len(cuts) == 16 and sum(n.startswith("text-cut") for n, _ in cuts) == 10
    zdict, _ = R.dict_inputs()
    for name, z in cuts:
        d = zlib.decompressobj()
        d.decompress(z)
        assert not d.eof, name
        with pytest.raises(D.DeflateError) as ei:
            D.deflate_decompress(z)
        assert ei.value.code == -D.E["E_LEN"], (name, ei.value.code)
        with pytest.raises(D.DeflateError) as ei:
            D.inflate_dict_host(z, zdict, "zlib")
        assert ei.value.code == -D.E["E_LEN"], (name, ei.value.code)
    for name, z in cuts:
        if name.startswith("zero-is-"):
            lt, lm = R._table(R.C.parse_dynamic_header(z)["ll"])
            sym = lt[0] >> 4
            want = {"literal": sym < 256, "length": sym > 256, "eob": sym == 256}[name.split("-")[2]]
            assert want, (name, sym)
