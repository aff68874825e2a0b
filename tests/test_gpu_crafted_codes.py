"""GPU tests (-m gpu): the Huffman stage held to prescribed histograms. tests/crafted_codes.py builds arrays whose stage-1 code stream
is chosen symbol by symbol — trees deeper than the 16- and 24-bit limits, massive ties, alphabets at the code-book paths' boundaries,
a thousand longest code words in a row — and every stage is compared with the numpy model (tests/szh_ref.py) and with the exact
length-limited optimum (package-merge): stage-1 codes, header, book (symbols, Kraft sum, limit, cost), chunk table, bit stream,
decode. Then the same stream goes through the alternative forms of the encoder, the decoder and a context's later calls.
tests/test_crafted_codes_cpu.py holds the families to their regimes without a GPU; profiles/r16_crafted_codes.txt has the figures.

What these streams found (profiles/r16_crafted_codes.txt has the figures before and after): every stage was exact, but where the 16-bit
limit binds cb_kraft_repair — whole leaves lengthened to the limit — cost 0.27 % of the stream on fib17, 0.31 % on fib17x56's exact book and
3.6 % (0.093 bit/symbol) on deep24-clustered in one-byte codes, against the 0.2 % of szh_ref.assert_book_optimal and the kernel's own
"< 0.01 bit/symbol". The small path now measures what the repair cost and takes the optimum by package-merge beyond 1 / 2048 of the stream
(cb_package_merge, sz3hip_kernels.hip): those books now equal the reference's cost."""
import functools
import types

import numpy as np
import pytest

import sz3_amd
import crafted_codes as cc
import payload_checks
import sampled_model
import szh_ref
from test_gpu_stages import _conf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

Dbg = sz3_amd.Dbg
EB = cc.EB
CASES = [(f, o, d, None) for f in cc.FAMILIES_1D for o in cc.ORDERS for d in ("f32", "f64")]
CASES += [(f, "shuffled", "f64", s) for f, s in sorted(cc.SHAPES_3D.items())]
CASES += [(cc.SAMPLED_FAMILY, o, "f32", cc.SAMPLED_SHAPE) for o in ("clustered", "shuffled")]  # the array of the sampled book
IDS = ["%s-%s-%s%s" % (f, o, d, "" if s is None else "-%dd" % len(s)) for f, o, d, s in CASES]

# encoder forms: (flags, the existing tests hold this form to the bytes of ...: None = its own payload is checked in full)
SAME_AS_DEFAULT, SAME_AS_EXACT = "default", "exact"
ENCODER_FORMS = [
    (Dbg.K1_NO_NARROW, SAME_AS_DEFAULT),                  # test_narrow_and_wide_code_paths_agree (a sampled book is the narrow form's alone)
    (Dbg.CB_NO_SAMPLED, None),
    (Dbg.PACK_OLD | Dbg.CB_NO_SAMPLED, SAME_AS_EXACT),    # test_pair_table_packer_writes_the_old_packers_bytes
    (Dbg.CB_ONE_CLASS, None),                             # (test_two_class_code_book_and_its_fallback: the two books differ)
    (Dbg.CB_SERIAL_MERGE, None),
    (Dbg.CB_NO_SPEC_WIDE, None),
    (Dbg.CTX_NO_MEMORY, None),
]
DECODER_FORMS = [Dbg.DEC_NO_FUSED_X, Dbg.DEC_NO_HALF, Dbg.DEC_CARRY_PASS]
FIGURES = []  # (case, form, one-byte codes?, symbols, limit, max_len, unlimited height, bits/symbol over package-merge, over the unlimited code, densest chunk's share of 1024 * limit bits)


def _calls(x, flags=0, spec=None, calls=3, base_flags=0):
    """a fresh context, `calls` compressions of x under `flags` (a context's second call on takes the one-launch forms and k_pack_b)
    -> (payloads, codes of the last call, stats of the last call, the last payload decoded under no flags)"""
    dev = torch.device("cuda:0")
    t = torch.from_numpy(x.copy()).to(dev)  # (the cached array is read-only)
    dc = sz3_amd.DeviceCompressor(x.size, x.dtype)
    if spec is not None:
        dc.set_speculation(spec, backoff=False)
    cap = dc.payload_bound(x.size, worst_case=True)
    pl = torch.empty(cap, dtype=torch.uint8, device=dev)
    out = []
    with sz3_amd.debug_flags(int(flags) | int(base_flags)):
        for _ in range(calls):
            size = dc.compress(_conf(x.shape, EB), t.data_ptr(), pl.data_ptr(), cap, 0)
            out.append(pl[:size].cpu().numpy().tobytes())
        codes = dc.debug_codes(x.size)
    st = dc.stats()
    dec = torch.empty_like(t)
    dc.decompress(pl.data_ptr(), size, dec.data_ptr(), 0)
    torch.cuda.synchronize()
    return out, codes, st, dec.cpu().numpy()


def _expected(prescribed, narrow):
    """-> (the codes stage 1 must emit, the places of the listed deltas): the prescribed stream — where stage 1 kept one-byte codes (its
    probe, 64 deltas every 32768 elements, met small deltas only: the clustered orders hide the far ones from it), a delta beyond
    +-127 is listed and coded as symbol 0, as szh_ref.dualquant(narrow=True) models it"""
    if not narrow:
        return prescribed, np.zeros(0, dtype=np.int64)
    far = np.abs(prescribed.astype(np.int64) - cc.RADIUS) > 127
    return np.where(far, 0, prescribed).astype(np.uint16), np.nonzero(far)[0]


def _check_payload(case, form, x, prescribed, blob, codes, st, dec):
    """everything the issue asks of one payload (tests/payload_checks.py); -> its header"""
    # stage 1: the prescribed codes; no value is listed, and a delta only where one-byte codes cannot hold it
    exp, listed = _expected(prescribed, st["narrow_codes"])
    # (the array of the sampled book in the default form: its book is held to the sample's counts, which numpy computes from the prescribed
    # deltas; the other forms of the encoder keep the rules they had: header, a valid prefix code)
    sample = None
    if form == "default" and st["narrow_codes"] and sampled_model.takes_sampled_book(x.shape, x.dtype, cc.RADIUS):
        sample = sampled_model.sample_counts(prescribed.astype(np.int64) - cc.RADIUS, x.shape)
    h, fig = payload_checks.check_payload(x, EB, exp, listed, prescribed[listed].astype(np.int64) - cc.RADIUS, np.zeros(0, dtype=np.int64), blob, codes, st, dec, sample=sample)
    FIGURES.append((case, form, fig["narrow"], fig["symbols"], fig["limit"], fig["max_len"], fig["height"], fig["over_pm"], fig["over_unlimited"], fig["densest"]))
    return h


@functools.lru_cache(maxsize=1)
def _base(case):
    """the case's array, its prescribed codes and the default form's three calls — computed once per case, read by its tests"""
    family, order, dtype, shape = case
    x, exp = cc.crafted(family, order, np.float32 if dtype == "f32" else np.float64, shape)
    cc.assert_prescribed(x, exp)  # precondition (a), before anything is launched
    # One-byte codes list every delta beyond +-127, and a stream lists at most max(1024, n / 8) of them (sz3hip_api.cpp, out_cap_limit:
    # beyond that the call is refused, test_one_byte_codes_refuse_what_they_cannot_list). A stream with more far deltas than that whose
    # probe meets none of them (flat2048, clustered) is shown to the Huffman stage in two-byte codes in every form.
    far = int(np.count_nonzero(np.abs(exp.astype(np.int64) - cc.RADIUS) > 127))
    base_flags = Dbg.K1_NO_NARROW if far > max(1024, x.size // 8) else 0
    blobs, codes, st, dec = _calls(x, base_flags=base_flags)
    return types.SimpleNamespace(x=x, exp=exp, blobs=blobs, codes=codes, st=st, dec=dec, name=IDS[CASES.index(case)], base_flags=base_flags)


def _stages(b):
    h = _check_payload(b.name, "default", b.x, b.exp, b.blobs[0], b.codes, b.st, b.dec)
    assert b.blobs[0] == b.blobs[1] == b.blobs[2], "a repeated call writes another payload"
    if b.x.shape == cc.SAMPLED_SHAPE:
        assert h["esc_sym"], "the array of the sampled book's size was coded without it"


def _encoder_forms(b):
    h0, _, _ = szh_ref.parse(b.blobs[0])
    exact = None
    for flags, same in ENCODER_FORMS:
        name = "|".join(f.name for f in Dbg if f & flags and f.name in ("K1_NO_NARROW", "CB_NO_SAMPLED", "PACK_OLD", "CB_ONE_CLASS", "CB_SERIAL_MERGE",
                                                                        "CB_NO_SPEC_WIDE", "CTX_NO_MEMORY"))
        blobs, codes, st, dec = _calls(b.x, flags, base_flags=b.base_flags)
        assert blobs[0] == blobs[1] == blobs[2], "%s: a repeated call writes another payload" % name
        if flags == Dbg.CB_NO_SAMPLED:
            exact = blobs[0]
        # (one-byte and two-byte codes give one payload unless the one-byte form has a sampled book or lists deltas the two-byte form codes)
        want = {SAME_AS_DEFAULT: None if h0["esc_sym"] or h0["n_dout"] else b.blobs[0], SAME_AS_EXACT: exact, None: None}[same]
        if want is not None:
            assert blobs[0] == want, "%s: not the bytes of the form it is held to" % name
        if blobs[0] == b.blobs[0]:
            assert np.array_equal(codes, b.codes) and np.array_equal(dec, b.dec)   # (the payload itself: the stages part)
        else:
            h = _check_payload(b.name, name, b.x, b.exp, blobs[0], codes, st, dec)
            assert not (flags & (Dbg.CB_NO_SAMPLED | Dbg.K1_NO_NARROW)) or not h["esc_sym"]


def _decoder_forms(b):
    dev = torch.device("cuda:0")
    pl = torch.from_numpy(np.frombuffer(b.blobs[0], dtype=np.uint8).copy()).to(dev)
    dc = sz3_amd.DeviceCompressor(b.x.size, b.x.dtype)
    for flags in DECODER_FORMS:
        out = torch.empty(b.x.shape, dtype=torch.float32 if b.x.dtype == np.float32 else torch.float64, device=dev)
        with sz3_amd.debug_flags(int(flags)):
            dc.decompress(pl.data_ptr(), pl.numel(), out.data_ptr(), 0)
            torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), b.dec), "decoder form %d: another array" % int(flags)


def _later_calls(b, spec):
    """the second and third call of one context — stage 2 with the previous call's book beside this call's, or never — write the first
    call's bytes (the stream is the same: the previous book IS this call's)"""
    blobs, codes, st, dec = _calls(b.x, spec=spec, base_flags=b.base_flags)
    assert blobs[0] == blobs[1] == blobs[2] == b.blobs[0]
    assert np.array_equal(codes, b.codes) and np.array_equal(dec, b.dec)


PARTS = {"stages": _stages, "encoder-forms": _encoder_forms, "decoder-forms": _decoder_forms,
         "later-calls-speculation": lambda b: _later_calls(b, True), "later-calls-no-speculation": lambda b: _later_calls(b, False)}


@pytest.mark.parametrize("part", list(PARTS))   # (the parts of a case one after the other: they share the case's array and default payload)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_crafted_stream(case, part):
    PARTS[part](_base(case))


def test_one_byte_codes_refuse_what_they_cannot_list():
    """flat2048, clustered: 5379 of 6144 deltas lie beyond +-127 and the probe's 64 deltas are all small. Stage 1 either takes two-byte codes
    or, having taken one-byte codes, refuses the array with SZ3HIP_EOUTLIERS (more listed deltas than a stream holds) — an error, not a
    fault; the context then codes the same array in two-byte codes"""
    x, exp = cc.crafted("flat2048", "clustered", np.float32)
    dev = torch.device("cuda:0")
    t = torch.from_numpy(x.copy()).to(dev)
    dc = sz3_amd.DeviceCompressor(x.size, x.dtype)
    cap = dc.payload_bound(x.size, worst_case=True)
    pl = torch.empty(cap, dtype=torch.uint8, device=dev)
    try:
        dc.compress(_conf(x.shape, EB), t.data_ptr(), pl.data_ptr(), cap, 0)
        assert dc.stats()["narrow_codes"] == 0
    except sz3_amd.SZ3HipError as e:
        assert e.code == -6
    with sz3_amd.debug_flags(int(Dbg.K1_NO_NARROW)):
        size = dc.compress(_conf(x.shape, EB), t.data_ptr(), pl.data_ptr(), cap, 0)
    assert np.array_equal(dc.debug_codes(x.size), exp)
    out = torch.empty_like(t)
    dc.decompress(pl.data_ptr(), size, out.data_ptr(), 0)
    torch.cuda.synchronize()
    assert float((out.double() - t.double()).abs().max()) <= EB
