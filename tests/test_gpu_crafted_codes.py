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
    """everything the issue asks of one payload; -> its header"""
    n = x.size
    # stage 1: the prescribed codes; no value is listed, and a delta only where one-byte codes cannot hold it
    exp, listed = _expected(prescribed, st["narrow_codes"])
    assert np.array_equal(codes, exp), "quantisation codes differ from the prescribed stream"
    h, o, sec = szh_ref.parse(blob)
    assert h["magic"] == szh_ref.MAGIC and h["n"] == n and h["payload_bytes"] == len(blob) == st["payload_bytes"]
    assert h["n_vout"] == 0 and h["n_dout"] == len(listed) and st["n_value_outliers"] == 0 and st["n_delta_outliers"] == len(listed)
    assert np.array_equal(sec["dout_idx"].astype(np.int64), listed)
    assert np.array_equal(sec["dout_val"].astype(np.int64), prescribed[listed].astype(np.int64) - cc.RADIUS)
    lens = sec["lens"].astype(np.int64)
    present = np.unique(exp)
    have = set((h["sym_min"] + np.nonzero(lens)[0]).tolist())
    freq = np.bincount(exp, minlength=65536)[h["sym_min"]:h["sym_min"] + h["sym_count"]].astype(np.int64)
    kraft_units = sum(1 << (szh_ref.MAX_LEN - int(l)) for l in lens[lens > 0])
    assert h["max_len"] == lens.max() == st["max_code_len"]
    if h["esc_sym"]:
        # the sampled book (test_gpu_sampled.py's header rules): a code word for every byte value, whatever the sample met — the clustered
        # order hides the rare run from it on purpose; a valid prefix code, no claim about its cost
        assert st["narrow_codes"] == 1 and n >= 1 << 22
        assert h["esc_sym"] == h["radius"] + 128 and h["sym_min"] == h["radius"] - 127 and h["sym_count"] == 256 and h["version"] == 5
        assert set(present.tolist()) <= have and h["esc_sym"] in have and freq.sum() == n
        assert kraft_units <= 1 << szh_ref.MAX_LEN and lens.max() <= szh_ref.MAX_LEN
        limit = szh_ref.MAX_LEN
        bfreq = freq
    else:
        assert h["version"] == 4
        book, filled = szh_ref.book_symbols(present)
        assert have == book, "the book's symbols are not the stream's (+ margins)"
        limit = szh_ref.SHORT_LEN if len(book) <= szh_ref.SHORT_SYMS else szh_ref.MAX_LEN
        assert kraft_units == 1 << szh_ref.MAX_LEN, "Kraft sum %d / 2^24" % kraft_units
        assert lens.max() <= limit
        bfreq, bmin, blimit = szh_ref.book_histogram(np.bincount(exp, minlength=65536)[present.min():present.max() + 1], int(present.min()))
        assert blimit == limit and freq.sum() == n
        if filled:
            assert h["sym_min"] == bmin == min(book) and h["sym_count"] == len(book) == len(bfreq)
            assert np.array_equal(np.maximum(freq, 1), bfreq)
        else:
            assert h["sym_min"] == bmin and h["sym_count"] == len(bfreq) and np.array_equal(freq, bfreq)
    # the book's cost: never below the length-limited optimum; the project's rule against the unlimited code; the kernel's documented loss
    pm = szh_ref.package_merge_lengths(bfreq, limit)
    pm_cost, gpu_cost = int((bfreq * pm).sum()), int((bfreq * lens).sum())
    unlimited, height = szh_ref.huffman_cost(bfreq)
    bits, chunkwords, subbits = szh_ref.chunk_table(exp, lens, h["sym_min"], h["esc_sym"])
    FIGURES.append((case, form, int(st["narrow_codes"]), len(bfreq), limit, int(lens.max()), height, (gpu_cost - pm_cost) / n, (gpu_cost - unlimited) / n, float(bits.max()) / (szh_ref.CHUNK * limit)))
    if not h["esc_sym"]:
        assert pm_cost <= gpu_cost, "the book costs less than the length-limited optimum: not a code of that limit"
        szh_ref.assert_book_optimal(bfreq, lens, limit)
        if len(bfreq) <= szh_ref.SHORT_SYMS:
            assert (gpu_cost - unlimited) / n < 0.01, "16-bit limit: %.5f bit/symbol over the unlimited code" % ((gpu_cost - unlimited) / n)
    # the packed stream: the chunk table of the whole payload from the payload's own lengths, the slow decoder on the densest, first and last chunk
    assert h["n_chunks"] == len(bits) and h["bitstream_words"] == int(chunkwords.sum())
    assert np.array_equal(sec["chunkwords"], chunkwords), "chunkwords differ from the lengths' sums"
    assert np.array_equal(sec["subbits"], subbits), "restart offsets differ from the lengths' sums"
    if n <= 120000:
        assert np.array_equal(szh_ref.huffman_decode(h, sec), exp), "the bit stream does not decode to the prescribed codes"
    else:
        pick = sorted({int(np.argmax(bits)), 0, h["n_chunks"] - 1})
        got = szh_ref.huffman_decode(h, sec, chunks=pick)
        for c in pick:
            sl = slice(c * szh_ref.CHUNK, (c + 1) * szh_ref.CHUNK)
            assert np.array_equal(got[sl], exp[sl]), "chunk %d does not decode to the prescribed codes" % c
    # the decode: the model's array bit for bit, within the bound
    model = szh_ref.reconstruct(h, sec, exp).reshape(x.shape)
    assert np.array_equal(dec, model), "the decoder's array differs from the model's"
    assert np.max(np.abs(dec.astype(np.float64) - x.astype(np.float64))) <= EB
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
