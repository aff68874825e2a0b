"""GPU tests (-m gpu): the wide code books held to prescribed histograms. tests/crafted_codes.py builds arrays
whose two-byte code stream has 300 .. 65 535 symbols with a chosen count each — the boundaries of the three constructions (cb_small,
codebook_wide<false>, codebook_wide<true>), both tiers of the two-class rule at and next to every threshold, trees deeper than the 16-
and the 24-bit limit on the wide path — and every payload is held to the numpy model of the format (tests/payload_checks.py) and of the
wide book's rules (tests/widebook_model.py): the tier, the octave, the class's weight and its floor, a complete code, the exact optimum
over the weights the construction runs on. Then the same stream goes through the alternative forms of the encoder and the decoder, a
context's later calls, and a context that has just seen another family. tests/test_widebook_model_cpu.py holds the families to their
regimes without a GPU; profiles/r28_wide_books.txt has the figures.

Two-byte codes. Stage 1 keeps one-byte codes where its probe (64 deltas of every 32768) meets few far deltas, lists the far ones and
codes at most 256 symbols: such a stream never reaches the wide book. Where the model of the probe (sampled_model.narrow_codes) says so
the case runs under Dbg.K1_NO_NARROW in every form (deep24w: its 1100 rare symbols are 1100 of 3.5 M deltas; the clustered orders
of the flat families); every case asserts two-byte codes."""
import functools
import types

import numpy as np
import pytest

import sz3_amd
import crafted_codes as cc
import payload_checks
import sampled_model
import szh_ref
import widebook_model as wm
from fields import field3d
from test_gpu_stages import _conf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

Dbg = sz3_amd.Dbg
EB = cc.EB
CASES = [(f, "balanced", d, None) for f in cc.WIDE_1D for d in ("f32", "f64")]
CASES += [(f, "clustered", d, None) for f in cc.FLAT_WIDE_CLUSTERED + ("tier1",) for d in ("f32", "f64")]  # runs of the longest code words from element 0 on
CASES += [(f, "balanced", "f64", s) for f, s in sorted(cc.WIDE_SHAPE_ND.items())]
IDS = ["%s-%s-%s%s" % (f, o, d, "" if s is None else "-%dd" % len(s)) for f, o, d, s in CASES]

# encoder forms: (flag, held to the default form's bytes?). CB_ONE_CLASS builds another book wherever the default is two-class: its own
# payload is checked in full against the ONE-class rules. CB_SERIAL_MERGE merges in another order: on ties it may give other lengths of
# the same cost — the default's bytes, or its own payload checked in full. The other three change how the book's launches are arranged,
# never the book: the default's bytes.
ENCODER_FORMS = [(Dbg.CB_ONE_CLASS, False), (Dbg.CB_COMPACT_IN_WG, True), (Dbg.CB_NO_SPEC_WIDE, True), (Dbg.CTX_NO_MEMORY, True), (Dbg.CB_SERIAL_MERGE, False)]
FORM_NAMES = {Dbg.CB_ONE_CLASS: "CB_ONE_CLASS", Dbg.CB_COMPACT_IN_WG: "CB_COMPACT_IN_WG", Dbg.CB_NO_SPEC_WIDE: "CB_NO_SPEC_WIDE", Dbg.CTX_NO_MEMORY: "CTX_NO_MEMORY",
              Dbg.CB_SERIAL_MERGE: "CB_SERIAL_MERGE"}   # (some bits have other meanings elsewhere, and other names with them)
DECODER_FORMS = [Dbg.DEC_NO_FUSED_X, Dbg.DEC_NO_HALF, Dbg.DEC_CARRY_PASS]
FIGURES = []  # one dict per checked payload (what profiles/r28_wide_books.txt records)


def _calls(x, flags=0, spec=None, calls=3, base_flags=0, dc=None):
    """a fresh context (or `dc`), `calls` compressions of x -> (payloads, codes, stats, decode of the last payload under no flags, context)"""
    dev = torch.device("cuda:0")
    t = torch.from_numpy(x.copy()).to(dev)
    dc = sz3_amd.DeviceCompressor(x.size, x.dtype) if dc is None else dc
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
    return out, codes, st, dec.cpu().numpy(), dc


def _check(b, form, blob, codes, st, dec, one_class=False):
    """the payload in full: the prescribed codes, no list, the wide book's rules; -> (header, figures)"""
    assert st["narrow_codes"] == 0, "the stream was coded in one-byte codes: not the wide book's"
    none = np.zeros(0, dtype=np.int64)
    h, fig = payload_checks.check_payload(b.x, EB, b.exp, none, none, none, blob, codes, st, dec, one_class=one_class)
    w = fig["wide"]
    if w is not None:
        r = w["rule"] or {}
        FIGURES.append(dict(case=b.name, form=form, symbols=w["symbols"], path=w["path"], tier=(r.get("keep"), r.get("k")) if r else None,
                            n_rare=r.get("n_rare", 0), rare_bits=r.get("rare_bits", 0), floor=r.get("floor_engaged"), len_cls=w["len_cls"],
                            max_len=w["max_len"], height=w["natural_height"], tree_height=w["height"], over_pm=(w["cost"] - w["pm_cost"]) / float(b.x.size),
                            over_tree=(w["cost"] - w["huffman_cost"]) / float(b.x.size), over_one_class=w["over_one_class"], densest=fig["densest"]))
    return h, fig


@functools.lru_cache(maxsize=1)
def _base(case):
    """the case's array, its prescribed codes and the default form's three calls on a fresh context — once per case, read by its parts"""
    family, order, dtype, shape = case
    x, exp = cc.crafted(family, order, np.float32 if dtype == "f32" else np.float64, shape)
    cc.assert_prescribed(x, exp)  # before anything is launched
    base_flags = Dbg.K1_NO_NARROW if sampled_model.narrow_codes(exp.astype(np.int64) - cc.RADIUS, cc.RADIUS) else 0
    blobs, codes, st, dec, _ = _calls(x, base_flags=base_flags)
    return types.SimpleNamespace(x=x, exp=exp, blobs=blobs, codes=codes, st=st, dec=dec, name=IDS[CASES.index(case)], base_flags=base_flags, family=family)


def _stages(b):
    h, fig = _check(b, "default", b.blobs[0], b.codes, b.st, b.dec)
    assert b.blobs[0] == b.blobs[1] == b.blobs[2], "a repeated call writes another payload"
    want = cc.WIDE_REGIME[b.family]
    if b.x.ndim == 1:  # (the 3-D case has more of the most frequent symbol than the family: its verdict is the model's all the same)
        assert (fig["wide"] is not None) == (want["path"] != "small")
    if fig["wide"] is not None:
        # the class rule's verdict is the payload's: the rare symbols share one length iff the model says two-class (check_wide_book
        # holds a two-class verdict to it; a one-class verdict to a complete code of the exact optimum, which a class code is not)
        rule = fig["wide"]["rule"]
        assert (rule is not None) == (want["tier"] is not None)
        if rule is not None:
            assert (rule["keep"], rule["k"]) == want["tier"] and rule["floor_engaged"] == want["floor"]
            assert (rule["n_rare"], rule["rare_bits"]) == (want["n_rare"], want["rare_bits"])
        assert fig["wide"]["limit_binds"] == want["binds"]


def _encoder_forms(b):
    for flags, same in ENCODER_FORMS:
        name = FORM_NAMES[flags]
        blobs, codes, st, dec, _ = _calls(b.x, flags, base_flags=b.base_flags)
        assert blobs[0] == blobs[1] == blobs[2], "%s: a repeated call writes another payload" % name
        if flags == Dbg.CB_ONE_CLASS:
            _check(b, name, blobs[0], codes, st, dec, one_class=True)  # the one-class rules: a complete code, the exact optimum
            h, _, sec = szh_ref.parse(b.blobs[0])
            freq = np.bincount(b.exp, minlength=65536)[h["sym_min"]:h["sym_min"] + h["sym_count"]]
            assert (blobs[0] == b.blobs[0]) == (wm.class_rule(freq) is None), "CB_ONE_CLASS and the default differ exactly where the default is two-class"
            continue
        if same:
            assert blobs[0] == b.blobs[0], "%s: not the default form's bytes" % name
        if blobs[0] == b.blobs[0]:
            assert np.array_equal(codes, b.codes) and np.array_equal(dec, b.dec)
        else:
            _check(b, name, blobs[0], codes, st, dec)


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
    blobs, codes, st, dec, _ = _calls(b.x, spec=spec, base_flags=b.base_flags)
    assert blobs[0] == blobs[1] == blobs[2] == b.blobs[0]
    assert np.array_equal(codes, b.codes) and np.array_equal(dec, b.dec)


PARTS = {"stages": _stages, "encoder-forms": _encoder_forms, "decoder-forms": _decoder_forms,
         "later-calls-speculation": lambda b: _later_calls(b, True), "later-calls-no-speculation": lambda b: _later_calls(b, False)}


@pytest.mark.parametrize("part", list(PARTS))   # (the parts of a case one after the other: they share the case's array and default payload)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_book(case, part):
    PARTS[part](_base(case))


def test_one_class_and_two_class_books_are_told_apart():
    """tier1: the CB_ONE_CLASS payload passes the one-class check and fails the two-class one; the default payload the other way round"""
    b = _base(("tier1", "balanced", "f32", None))
    blobs, codes, st, dec, _ = _calls(b.x, Dbg.CB_ONE_CLASS, calls=1)
    assert blobs[0] != b.blobs[0]
    _check(b, "CB_ONE_CLASS", blobs[0], codes, st, dec, one_class=True)
    with pytest.raises(AssertionError, match="rare class|Kraft"):
        _check(b, "CB_ONE_CLASS", blobs[0], codes, st, dec)
    _check(b, "default", b.blobs[0], b.codes, b.st, b.dec)
    with pytest.raises(AssertionError, match="Kraft"):
        _check(b, "default", b.blobs[0], b.codes, b.st, b.dec, one_class=True)


# (the array, what spec_stats must count: 0 nothing, +1 a hit, -1 a miss) per call of the shared context
AFTER_ANOTHER = {
    # flat640 leaves cb_part = 0 and 640 symbols: neither speculative form of stage 2 is taken after it. tier1 then meets the classic book
    # launch in the form predicted from flat640 (part_hint 0): that form declines, raises `mispredict`, and stage 2 is repeated with both
    # forms — no speculation was made, none is counted. tier1 again: the wide book on its own stream, a hit. flat640 after tier1: the
    # wide form launched alone meets the small form's alphabet — a miss, stage 2 repeated.
    "flat640-tier1": [("a", 0), ("a", 0), ("b", 0), ("b", +1), ("a", -1), ("a", 0)],
    "tier1-flat640": [("a", 0), ("a", +1), ("b", -1), ("b", 0), ("a", 0), ("a", +1)],
}


@pytest.mark.parametrize("pair", sorted(AFTER_ANOTHER))
def test_context_after_another_family(pair):
    """one context through two families whose books come from different launches (flat640: cb_small; tier1: the two-class wide form) — the
    mispredicted part_hint in both directions, where stage 2 is repeated: every payload is a fresh context's, and spec_stats counts a hit
    on the repeated wide array and a miss on the change away from it (AFTER_ANOTHER)"""
    first, then = pair.split("-")
    xs = {"a": cc.crafted(first, "balanced", np.float32)[0], "b": cc.crafted(then, "balanced", np.float32)[0]}
    for f, k in ((first, "a"), (then, "b")):
        cc.assert_prescribed(xs[k], cc.crafted(f, "balanced", np.float32)[1])
    n = max(x.size for x in xs.values())
    dev = torch.device("cuda:0")
    shared = sz3_amd.DeviceCompressor(n, np.float32)
    shared.set_speculation(True, backoff=False)
    shared.set_deterministic(True)
    cap = shared.payload_bound(n, worst_case=True)
    pl = torch.empty(cap, dtype=torch.uint8, device=dev)

    def run(dc, x):
        t = torch.from_numpy(x.copy()).to(dev)
        with sz3_amd.debug_flags(int(Dbg.K1_NO_NARROW)):  # (flat640 has 1920 elements: the probe sees its first 64 alone)
            size = dc.compress(_conf(x.shape, EB), t.data_ptr(), pl.data_ptr(), cap, 0)
        torch.cuda.synchronize()
        assert dc.stats()["narrow_codes"] == 0
        return pl[:size].cpu().numpy().tobytes()

    fresh = {k: run(sz3_amd.DeviceCompressor(n, np.float32), x) for k, x in xs.items()}
    for step, (k, want) in enumerate(AFTER_ANOTHER[pair]):
        h0, m0 = shared.spec_stats()
        got = run(shared, xs[k])
        h1, m1 = shared.spec_stats()
        assert got == fresh[k], "step %d: the payload depends on the context's history" % step
        assert (h1 - h0, m1 - m0) == {0: (0, 0), 1: (1, 0), -1: (0, 1)}[want], "step %d: hits %d misses %d" % (step, h1 - h0, m1 - m0)


INTERP_SHAPE = (96, 96, 96)


def test_interpolation_stream_has_a_two_class_book():
    """ALGO_INTERP, f32, bound 1e-5, field3d at 96^3 — the smallest cube tried whose stream has more than 4096 symbols: the book from
    debug_codes' histogram, the chunk table and the slow decoder. szk_launch_encode packs the context's code array from element 0 on,
    1024 codes a chunk, and debug_codes copies that array as it lies: the packer reads the codes in debug_codes' order, so the chunk table
    and the picked chunks are checked too."""
    a = field3d(INTERP_SHAPE)
    dev = torch.device("cuda:0")
    t = torch.from_numpy(a).to(dev)
    dc = sz3_amd.DeviceCompressor(a.size, a.dtype)
    cap = dc.payload_bound(a.size, worst_case=True)
    pl = torch.empty(cap, dtype=torch.uint8, device=dev)
    conf = sz3_amd.Config(*a.shape)
    conf.cmprAlgo = sz3_amd.ALGO_INTERP
    conf.absErrorBound = 1e-5
    size = dc.compress(conf, t.data_ptr(), pl.data_ptr(), cap, 0)
    codes = dc.debug_codes(a.size)
    out = torch.empty_like(t)
    dc.decompress(pl.data_ptr(), size, out.data_ptr(), 0)
    torch.cuda.synchronize()
    assert float((out.double() - t.double()).abs().max()) <= 1e-5
    h, _, sec = szh_ref.parse(pl[:size].cpu().numpy().tobytes())
    symbols = int(np.count_nonzero(np.bincount(codes, minlength=65536)))
    assert symbols > wm.CB_CLASS_MIN, "the interpolation stream of %s has %d symbols: not a wide alphabet" % (INTERP_SHAPE, symbols)
    assert h["predictor"] == 1 and h["n"] == a.size
    fig = payload_checks.check_book_and_stream(h, sec, codes, a.size)
    w = fig["wide"]
    assert w is not None and w["path"] == wm.WIDE2
    FIGURES.append(dict(case="interp-%dx%dx%d" % INTERP_SHAPE, form="default", symbols=w["symbols"], path=w["path"],
                        tier=(w["rule"]["keep"], w["rule"]["k"]) if w["rule"] else None, n_rare=(w["rule"] or {}).get("n_rare", 0),
                        rare_bits=(w["rule"] or {}).get("rare_bits", 0), floor=(w["rule"] or {}).get("floor_engaged"), len_cls=w["len_cls"],
                        max_len=w["max_len"], height=w["natural_height"], tree_height=w["height"], over_pm=(w["cost"] - w["pm_cost"]) / float(a.size),
                        over_tree=(w["cost"] - w["huffman_cost"]) / float(a.size), over_one_class=w["over_one_class"], densest=fig["densest"]))
