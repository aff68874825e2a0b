"""GPU tests (-m gpu) of the shared code book under the histogram exchange, on contexts that have a history.

The slab-parallel design rests on one property: between stage 1 and stage 2 every rank's code histogram is replaced by the sum over
all ranks, and every rank codes with the one book built from that sum. A context's later calls take shortcuts its first call does
not (one-byte forms, speculated books and hand-over decisions, the sampled book); a shortcut that is repeated inside finish() after the
exchange runs stage 1 again, which refills the histogram with local counts and codes the slab with a local book — the payload still
decodes, only the book is no longer shared and the caller's buffer is overwritten.

Here R ranks are simulated on one GPU in one process: R DeviceCompressors, each with a caller-owned int64[65536] histogram
(set_histogram), stage 1 on every rank, every tensor set to the sum of all of them on the stream, then stage 2 and finish on every
rank. The measured call follows a history (a priming call of the same or another kind of data, shape or mode) and must give the
bytes R fresh contexts give. The fresh contexts' payloads are checked against references computed here: one book, the true summed
histogram, a book as good as a heapq Huffman code over it, values bit-identical to a non-exchanging context's and within the bound.
The host API's own exchange (conf.openmp) is checked against a fresh child process."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import sz3_amd  # noqa: E402
import szh_ref  # noqa: E402
from fields import field1d, field2d, field3d, field4d  # noqa: E402
from oracle_binding import oracle  # noqa: E402
from sz3_amd import distributed as D  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BINS = 65536
DECODE_MAX = 120000   # slabs up to this many elements: codes from the pure-python decoder of the payload (else debug_codes)
BLOCK_RECON_MAX = 12000  # block streams up to this many elements: the slow block-by-block host reconstruction too


def _noise(shape, sigma, dtype, seed=11):
    return np.random.default_rng(seed).normal(0.0, sigma, shape).astype(dtype)


def _lorenzo(l1=1, l2=0, reg=0):
    return dict(cmprAlgo=sz3_amd.ALGO_LORENZO_REG, lorenzo=l1, lorenzo2=l2, regression=reg)


INTERP = dict(cmprAlgo=sz3_amd.ALGO_INTERP)
INTERP_LORENZO = dict(cmprAlgo=sz3_amd.ALGO_INTERP_LORENZO)


# (name, ranks, eb, config fields, smooth array, rough array, which one is measured)
# smooth: noise of the field near the bound (one-byte codes; lorenzo+regression: every block takes Lorenzo, the plain stream)
# rough: noise far above the bound (two-byte codes, another alphabet; lorenzo+regression: regression blocks, the block stream)
def _cases():
    f32, f64 = np.float32, np.float64
    c = []
    for dt, eb in ((f32, 1e-3), (f64, 1e-4)):
        t = "f32" if dt == f32 else "f64"
        c += [
            ("lor1-1d-" + t, 3, eb, _lorenzo(), lambda dt=dt: field1d(150001, dt), lambda dt=dt: field1d(150001, dt) + _noise(150001, 0.05, dt), "smooth"),
            ("lor1-2d-" + t, 2, eb, _lorenzo(), lambda dt=dt: field2d((300, 417), dt), lambda dt=dt: field2d((300, 417), dt) + _noise((300, 417), 0.05, dt), "smooth"),
            ("lor1-3d-" + t, 4, eb, _lorenzo(), lambda dt=dt: field3d((40, 48, 64), dt), lambda dt=dt: field3d((40, 48, 64), dt) + _noise((40, 48, 64), 0.05, dt), "smooth"),
            ("lor1-4d-" + t, 2, 10 * eb, _lorenzo(), lambda dt=dt: field4d((8, 12, 14, 20), dt),
             lambda dt=dt: field4d((8, 12, 14, 20), dt) + _noise((8, 12, 14, 20), 0.5, dt), "smooth"),
        ]
    s3 = (36, 64, 96)
    s2 = (256, 512)
    c += [
        ("lor2-3d", 2, 1e-3, _lorenzo(0, 1, 0), lambda: field3d((40, 48, 64)), lambda: field3d((40, 48, 64)) + _noise((40, 48, 64), 0.05, f32), "smooth"),
        # the block hand-over decision flips between the priming call and the measured one, both ways (2-D and 3-D)
        ("lr-2d-to-block", 2, 1e-3, _lorenzo(1, 0, 1), lambda: field2d(s2), lambda: _noise(s2, 0.05, f32), "rough"),
        ("lr-2d-to-plain", 2, 1e-3, _lorenzo(1, 0, 1), lambda: field2d(s2), lambda: _noise(s2, 0.05, f32), "smooth"),
        ("lr-3d-to-block", 2, 1e-3, _lorenzo(1, 0, 1), lambda: field3d(s3), lambda: _noise(s3, 0.05, f32), "rough"),
        ("lr-3d-to-plain", 2, 1e-3, _lorenzo(1, 0, 1), lambda: field3d(s3), lambda: _noise(s3, 0.05, f32), "smooth"),
        ("lr-3d-to-block-f64", 3, 1e-4, _lorenzo(1, 0, 1), lambda: field3d(s3, f64), lambda: _noise(s3, 0.005, f64), "rough"),
        # 1-D and 4-D: no selection pass, the fit pass chooses
        ("lr-1d", 2, 1e-3, _lorenzo(1, 0, 1), lambda: field1d(100003), lambda: field1d(100003) + _noise(100003, 0.05, f32), "smooth"),
        ("lr-4d", 2, 1e-2, _lorenzo(1, 0, 1), lambda: field4d((8, 12, 12, 18)), lambda: _noise((8, 12, 12, 18), 0.5, f32), "smooth"),
        ("interp-3d", 2, 1e-3, INTERP, lambda: field3d((40, 48, 64)), lambda: field3d((40, 48, 64)) + _noise((40, 48, 64), 0.05, f32), "smooth"),
        ("interp-lorenzo-3d", 2, 1e-3, INTERP_LORENZO, lambda: field3d((40, 48, 64)), lambda: field3d((40, 48, 64)) + _noise((40, 48, 64), 0.05, f32), "smooth"),
        # more than 512 symbols in the summed histogram: the 24-bit length limit
        ("wide-alphabet", 2, 1e-3, _lorenzo(), lambda: field3d((48, 64, 64)) + _noise((48, 64, 64), 0.12, f32),
         lambda: field3d((48, 64, 64)) + _noise((48, 64, 64), 0.6, f32), "smooth"),
        # slabs of 2^22 elements in rows of 256: where a context that does not exchange takes the sampled book
        ("sampled-size", 2, 1e-3, _lorenzo(), lambda: field3d((128, 256, 256)), lambda: field3d((128, 256, 256)) + _noise((128, 256, 256), 0.05, f32), "smooth"),
    ]
    return c


CASES = _cases()
# priming histories before the measured call (every one an exchange call of all ranks): none (fresh contexts, the reference), the
# smooth / rough array of the same shape, another shape, the deterministic and speculation switches turned between the two calls,
# and the measured call itself twice in a row
HISTORIES = ["smooth", "rough", "shape", "modes", "modes-back", "twice"]


class Ranks:
    """R device contexts that exchange their histograms through caller-owned tensors"""

    def __init__(self, R, dtype, max_elems, confs):
        self.dev = torch.device("cuda:0")
        self.dcs = [sz3_amd.DeviceCompressor(max_elems, dtype) for _ in range(R)]
        self.hists = [torch.zeros(BINS, dtype=torch.int64, device=self.dev) for _ in range(R)]
        for dc, h in zip(self.dcs, self.hists):
            dc.set_histogram(h.data_ptr())
        self.cap = max(dc.payload_bound_conf(c, worst_case=True) for dc in self.dcs[:1] for c in confs)
        self.pls = [torch.empty(self.cap, dtype=torch.uint8, device=self.dev) for _ in range(R)]

    def call(self, confs, slabs):
        s = torch.cuda.current_stream().cuda_stream
        for dc, c, t in zip(self.dcs, confs, slabs):
            dc.stage1(c, t.data_ptr(), s)
        total = torch.stack(self.hists).sum(0)   # (the all-reduce: ordered on the stream between the stages)
        for h in self.hists:
            h.copy_(total)
        for dc, pl in zip(self.dcs, self.pls):
            dc.stage2(pl.data_ptr(), self.cap, s)
        sizes = [dc.finish(s) for dc in self.dcs]
        torch.cuda.synchronize()
        payloads = [pl[:n].cpu().numpy().tobytes() for pl, n in zip(self.pls, sizes)]
        return payloads, [h.cpu().numpy() for h in self.hists]


def _split(a, R):
    """the slabs along dims[0] (distributed.slab_bounds), on the device"""
    out = []
    for r in range(R):
        lo, hi = D.slab_bounds(a.shape[0], R, r)
        out.append(np.ascontiguousarray(a[lo:hi]))
    return out


def _conf(shape, eb, fields):
    c = sz3_amd.Config(*shape)
    c.errorBoundMode = sz3_amd.EB_ABS
    c.absErrorBound = eb
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def _other_shape(a, R):
    """a smaller array of another shape (fewer slices, and a shorter fastest dimension when there is more than one)"""
    sl = [slice(0, a.shape[0] - R)] + [slice(None)] * (a.ndim - 1)
    if a.ndim > 1:
        sl[-1] = slice(0, a.shape[-1] - 1)
    return np.ascontiguousarray(a[tuple(sl)])


def _codes(h, sec, dc, n):
    return szh_ref.huffman_decode(h, sec) if n <= DECODE_MAX else dc.debug_codes(n)


@pytest.mark.parametrize("name,R,eb,fields,smooth,rough,measured", CASES, ids=[c[0] for c in CASES])
def test_exchanged_code_book_is_shared_and_history_free(name, R, eb, fields, smooth, rough, measured):
    a_smooth, a_rough = smooth(), rough()
    a_meas = a_smooth if measured == "smooth" else a_rough
    dtype = a_meas.dtype
    dev = torch.device("cuda:0")
    arrays = {"smooth": a_smooth, "rough": a_rough, "shape": _other_shape(a_smooth, R)}
    slabs = {k: _split(v, R) for k, v in arrays.items()}
    dslabs = {k: [torch.from_numpy(x).to(dev) for x in v] for k, v in slabs.items()}
    confs = {k: [_conf(x.shape, eb, fields) for x in v] for k, v in slabs.items()}
    max_elems = max(x.size for v in slabs.values() for x in v)
    all_confs = [c for v in confs.values() for c in v]
    mk = measured

    # ---- the reference: R fresh contexts, one exchange call -----------------------------------------------------------------
    fresh = Ranks(R, dtype, max_elems, all_confs)
    ref, ref_hists = fresh.call(confs[mk], dslabs[mk])
    parsed = [szh_ref.parse(p) for p in ref]
    h0, _, s0 = parsed[0]
    for h, _, sec in parsed:  # one book everywhere, never a sampled one
        assert (h["sym_min"], h["sym_count"]) == (h0["sym_min"], h0["sym_count"]) and np.array_equal(sec["lens"], s0["lens"]), "ranks code with different books"
        assert h["esc_sym"] == 0, "a rank that exchanges its histogram took the sampled book"
    codes = []
    for r, (h, _, sec) in enumerate(parsed):
        n = slabs[mk][r].size
        assert h["n"] == n
        c = _codes(h, sec, fresh.dcs[r], n)
        if r == 0 and n <= DECODE_MAX:  # debug_codes against the payload's own codes (as counts: block streams store them block by block)
            dbg = fresh.dcs[r].debug_codes(n)
            assert np.array_equal(np.bincount(dbg, minlength=BINS), np.bincount(c, minlength=BINS))
            if h["predictor"] == 0:
                assert np.array_equal(dbg, c)
        codes.append(c)
    total = sum(np.bincount(c, minlength=BINS).astype(np.int64) for c in codes)
    for hr in ref_hists:
        assert np.array_equal(hr, total), "the histogram after finish() is not the sum over the ranks"
    # the book is optimal for the summed histogram (the rules of test_gpu_stages.py: margins of small alphabets, length limits)
    present = np.nonzero(total)[0]
    book, filled = szh_ref.book_symbols(present)
    lens = s0["lens"]
    if len(present) > 1:
        assert set((h0["sym_min"] + np.nonzero(lens)[0]).tolist()) == book
        limit = szh_ref.SHORT_LEN if len(book) <= szh_ref.SHORT_SYMS else szh_ref.MAX_LEN
        assert abs(szh_ref.kraft(lens) - 1.0) < 1e-9 and lens.max() == h0["max_len"] <= limit
        freq = total[h0["sym_min"]:h0["sym_min"] + h0["sym_count"]]
        if filled:
            assert h0["sym_min"] == min(book) and h0["sym_count"] == len(book)
            freq = np.maximum(freq, 1)
        szh_ref.assert_book_optimal(freq, lens, limit)
    if name == "wide-alphabet":
        assert len(book) > szh_ref.SHORT_SYMS, "the case must exercise the 24-bit limit"
    # values: within the bound, and what a context that does not exchange reconstructs, bit for bit
    for r in range(R):
        a, t, h, sec = slabs[mk][r], dslabs[mk][r], parsed[r][0], parsed[r][2]
        out = torch.empty_like(t)
        fresh.dcs[r].decompress(fresh.pls[r].data_ptr(), len(ref[r]), out.data_ptr(), 0)
        alone = sz3_amd.DeviceCompressor(a.size, dtype)
        cap = alone.payload_bound_conf(confs[mk][r], worst_case=True)
        pl = torch.empty(cap, dtype=torch.uint8, device=dev)
        n1 = alone.compress(confs[mk][r], t.data_ptr(), pl.data_ptr(), cap, 0)
        out1 = torch.empty_like(t)
        alone.decompress(pl.data_ptr(), n1, out1.data_ptr(), 0)
        torch.cuda.synchronize()
        dec, dec1 = out.cpu().numpy(), out1.cpu().numpy()
        assert float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= eb
        assert np.array_equal(dec.view(np.uint8), dec1.view(np.uint8)), "the exchanged book changed reconstructed values"
        if name == "sampled-size":
            own = szh_ref.parse(pl[:n1].cpu().numpy().tobytes())[0]
            assert own["esc_sym"] != 0, "the case must lie where a context that does not exchange takes the sampled book"
        if h["predictor"] == 0:
            model = szh_ref.reconstruct(h, sec, codes[r]).reshape(a.shape)
            assert np.array_equal(dec.view(np.uint8), model.view(np.uint8))
        elif h["predictor"] == 2 and a.size <= BLOCK_RECON_MAX:
            model, _ = szh_ref.reconstruct_blocks(h, sec, codes[r])
            assert np.array_equal(dec.reshape(-1).view(np.uint8), model.view(np.uint8))
        del alone

    # ---- the same exchange after a history: byte-identical payloads, the summed histogram in every caller's tensor ----------
    for hist in HISTORIES:
        ranks = Ranks(R, dtype, max_elems, all_confs)
        prime = {"smooth": "smooth", "rough": "rough", "shape": "shape", "modes": "smooth", "modes-back": "rough", "twice": mk}[hist]
        if hist == "modes":
            for dc in ranks.dcs:
                dc.set_deterministic(True)
                dc.set_speculation(False)
        elif hist == "modes-back":
            for dc in ranks.dcs:
                dc.set_speculation(True, backoff=False)
        primed, _ = ranks.call(confs[prime], dslabs[prime])
        if hist == "modes":
            for dc in ranks.dcs:
                dc.set_deterministic(False)
                dc.set_speculation(True)
        elif hist == "modes-back":
            for dc in ranks.dcs:
                dc.set_deterministic(True)
                dc.set_speculation(False)
        got, hists = ranks.call(confs[mk], dslabs[mk])
        if name.startswith("lr-2d-to-") or name.startswith("lr-3d-to-"):
            # the flip cases check their own setup: the priming call and the measured one took different predictors
            want = {"smooth": 0, "rough": 2}
            if prime in want:
                assert [szh_ref.parse(p)[0]["predictor"] for p in primed] == [want[prime]] * R, (hist, "priming predictor")
            assert [szh_ref.parse(p)[0]["predictor"] for p in got] == [want[mk]] * R, (hist, "measured predictor")
        for r in range(R):
            assert got[r] == ref[r], "%s: rank %d's payload differs from a fresh context's (%d vs %d bytes)" % (hist, r, len(got[r]), len(ref[r]))
            assert np.array_equal(hists[r], total), "%s: rank %d's histogram after finish() is not the sum over the ranks" % (hist, r)
        del ranks


# ---- the host API's own exchange (conf.openmp): slots are process-global and reused -------------------------------------------
def _unzstd(blob):
    """[u64 rawLen][zstd frames] -> raw bytes (the oracle's libzstd binding; checker only)"""
    L = oracle()
    rawlen, = struct.unpack_from("<Q", blob, 0)
    src = np.frombuffer(blob, dtype=np.uint8).copy()
    out = np.empty(rawlen, dtype=np.uint8)
    assert L.szo_zstd_decompress(src.ctypes.data, src.size, out.ctypes.data, rawlen) == rawlen
    return out.tobytes()


def _payload(stream):
    """single-slab SZ3 stream -> its payload (the blob between the 16-byte header and the Config trailer)"""
    b = bytes(stream)
    plen, = struct.unpack_from("<Q", b, 8)
    return b[16:16 + plen]


CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import sz3_amd
a = np.load(sys.argv[1])
conf = sz3_amd.Config(*a.shape)
conf.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
conf.errorBoundMode = sz3_amd.EB_ABS
conf.absErrorBound = float(sys.argv[3])
conf.regression = int(sys.argv[4])
conf.openmp = int(sys.argv[5])
blob, _ = sz3_amd.compress(a, conf)
open(sys.argv[2], "wb").write(blob.tobytes())
"""


def _host_conf(shape, eb, regression, openmp):
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
    c.errorBoundMode = sz3_amd.EB_ABS
    c.absErrorBound = eb
    c.regression = regression
    c.openmp = openmp
    return c


def _fresh_process(tmp_path, a, eb, regression, openmp):
    """the same host call in a child process whose slots have never coded anything"""
    script = tmp_path / "child.py"
    script.write_text(CHILD % ROOT)
    inp, out = tmp_path / "in.npy", tmp_path / "out.bin"
    np.save(inp, a)
    r = subprocess.run([sys.executable, str(script), str(inp), str(out), repr(eb), str(regression), str(openmp)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_bytes()


def test_openmp_call_after_an_openmp_call_whose_blocks_went_the_other_way(tmp_path, monkeypatch):
    """conf.openmp with lorenzo+regression: A (every block Lorenzo, the plain stream) then B (regression blocks) on the same pooled
    slots. B's slabs share one book, and B's container is the one a fresh process writes."""
    monkeypatch.setenv("SZ3HIP_SLABS", "2")
    shape, eb = (36, 64, 96), 1e-3
    A = field3d(shape)
    B = _noise(shape, 0.05, np.float32)
    blob_a, _ = sz3_amd.compress(A, _host_conf(shape, eb, 1, 1))
    blob_b, _ = sz3_amd.compress(B, _host_conf(shape, eb, 1, 1))
    _, _, blobs_a = D.split_container(blob_a.tobytes())
    _, _, blobs_b = D.split_container(blob_b.tobytes())
    ha = [szh_ref.parse(_unzstd(b))[0] for b in blobs_a]
    pb = [szh_ref.parse(_unzstd(b)) for b in blobs_b]
    assert [h["predictor"] for h in ha] == [0, 0] and [p[0]["predictor"] for p in pb] == [2, 2], "the case must flip the hand-over"
    (h0, _, s0), (h1, _, s1) = pb
    assert (h0["sym_min"], h0["sym_count"]) == (h1["sym_min"], h1["sym_count"]) and np.array_equal(s0["lens"], s1["lens"]), "B's slabs code with different books"
    dec, _ = sz3_amd.decompress(blob_b, np.float32, shape)
    assert float(np.max(np.abs(dec.astype(np.float64) - B.astype(np.float64)))) <= eb
    assert blob_b.tobytes() == _fresh_process(tmp_path, B, eb, 1, 1), "B's container depends on what the slots coded before"


def test_plain_call_after_an_openmp_call_is_a_fresh_slots_call(tmp_path, monkeypatch):
    """an openmp call leaves no exchange mark on the pooled slots: a plain call of a 2^22-element f32 Lorenzo array afterwards takes the
    sampled book and writes the bytes a fresh process writes. (The openmp call's slabs are as large as the plain call's array: a slot
    whose context is too small for a call gets a new one, which would hide a mark left on the old.)"""
    monkeypatch.setenv("SZ3HIP_SLABS", "2")
    shape, eb = (128, 256, 256), 1e-3
    blob_a, _ = sz3_amd.compress(field3d(shape), _host_conf(shape, eb, 0, 1))
    _, _, blobs_a = D.split_container(blob_a.tobytes())
    # (the openmp call itself: its slabs of 2^22 elements share one book, not a sampled one each — the mark is set before stage 1)
    (h0, _, s0), (h1, _, s1) = [szh_ref.parse(_unzstd(b)) for b in blobs_a]
    assert h0["esc_sym"] == 0 and h1["esc_sym"] == 0, "a slab of an openmp call took the sampled book"
    assert (h0["sym_min"], h0["sym_count"]) == (h1["sym_min"], h1["sym_count"]) and np.array_equal(s0["lens"], s1["lens"])
    big = field3d((64, 256, 256))
    blob, _ = sz3_amd.compress(big, _host_conf(big.shape, eb, 0, 0))
    h = szh_ref.parse(_unzstd(_payload(blob.tobytes())))[0]
    assert h["predictor"] == 0 and h["esc_sym"] != 0, "the plain call after an openmp call did not take the sampled book"
    assert blob.tobytes() == _fresh_process(tmp_path, big, eb, 0, 0), "the plain call's bytes depend on an earlier openmp call"
