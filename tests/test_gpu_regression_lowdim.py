"""GPU tests (-m gpu) of the block-composed predictor on arrays of one and two dimensions (sz3hip_regress.hip, k_blkn_*):
Lorenzo-1 / linear regression per block of 128 values (1-D) or 16 x 16 (2-D) — RegressionPredictor.hpp:22-55 (generic N),
ComposedPredictor.hpp:25-40 over BlockwiseIterator.hpp:151-184, default block sizes Config.hpp:175; SURVEY.md 8(d) C1 names this
predictor set (ALGO_LORENZO_REG defaults on a 1-D array).

Parity bar as in test_gpu_regression.py: strict bound; the stream read back by the numpy model of the block decoder bit for bit;
ratio and per-block selection against the oracle (the CPU restatement pinned to the reference)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sz3_amd  # noqa: E402
import szh_ref  # noqa: E402
from fields import field1d, field2d  # noqa: E402
from oracle_binding import make_config, oracle_compress, oracle_selection  # noqa: E402
from test_gpu_regression import MASKS, NO_EXIT, Dbg, _block_streams_wanted, _conf, _payload_of  # noqa: E402,F401  (the autouse fixture: block streams wanted)


def _field(shape, dtype):
    return field1d(shape[0], dtype) if len(shape) == 1 else field2d(shape, dtype)


@pytest.mark.parametrize("mask", ["R", "L1+R"])
@pytest.mark.parametrize("dtype,shape,eb,block", [(np.float32, (5000,), 1e-3, None), (np.float64, (3001,), 2e-2, 64), (np.float32, (130,), 1e-2, 7),
                                                 (np.float32, (70, 90), 1e-2, None), (np.float64, (33, 47), 2e-2, 8),
                                                 (np.float32, (64, 96), 5e-2, 32), (np.float32, (5, 200), 1e-3, 4)])
def test_low_dimensional_block_stream_against_the_numpy_model(mask, dtype, shape, eb, block):
    """ragged last blocks in every dimension: bound, header, and the numpy block decoder reproduces the GPU's reconstruction bit
    for bit from the stream (selection bits, coefficient deltas with the N + 1 divisor, codes, outlier lists)"""
    a = _field(shape, dtype)
    conf = _conf(shape, eb, *MASKS[mask], block=block)
    blob, ratio = sz3_amd.compress(a, conf)
    dec, c2 = sz3_amd.decompress(blob, dtype, shape)
    assert float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= eb
    if c2.cmprAlgo == sz3_amd.ALGO_LOSSLESS:
        pytest.skip("tiny field went lossless")
    h, o, sec = szh_ref.parse(_payload_of(blob))
    default = 128 if len(shape) == 1 else 16
    assert h["predictor"] == 2 and h["ndim"] == len(shape) and h["blk_edge"] == (block or default)
    assert h["blk_mask"] == sum(b << i for i, b in enumerate(MASKS[mask]))
    assert (c2.lorenzo, c2.lorenzo2, c2.regression) == MASKS[mask]
    codes = szh_ref.huffman_decode(h, sec)
    model, sel = szh_ref.reconstruct_blocks(h, sec, codes)
    assert np.array_equal(model.reshape(shape), dec), "numpy model of the block decoder and the GPU decoder disagree"
    assert set(np.unique(sel)) <= {0, 2}
    if mask == "L1+R":
        print(shape, "regression blocks: %.3f" % float((np.asarray(sel) == 2).mean()))
    # the encoder without the selection pass in front (development switch Dbg.BLK_NO_SELECT: the fit pass chooses and leaves q~ of every
    # element in the work array, the code pass reads it back) writes the same stream
    try:
        sz3_amd.lib().sz3hip_debug_flags(NO_EXIT | Dbg.BLK_NO_SELECT)
        blob2, _ = sz3_amd.compress(a, conf)
    finally:
        sz3_amd.lib().sz3hip_debug_flags(NO_EXIT)
    assert _payload_of(blob2) == _payload_of(blob)


@pytest.mark.parametrize("shape", [(40000,), (150, 260)])
def test_unpredictable_values_and_wide_deltas_in_low_dimensional_block_streams(shape):
    a = _field(shape, np.float32)
    flat = a.reshape(-1)
    flat[5] = np.nan
    flat[1234] = np.inf
    if len(shape) == 1:
        a[2000:2300] += 500.0  # a step: Lorenzo deltas beyond the radius next to it, regression residuals unpredictable
    else:
        a[40:75, 50:120] += 500.0
    for mask in ("L1+R", "R"):
        conf = _conf(shape, 1e-3, *MASKS[mask])
        conf.quantbinCnt = 1024
        blob, _ = sz3_amd.compress(a, conf)
        dec, _ = sz3_amd.decompress(blob, np.float32, shape)
        ok = np.isfinite(a)
        assert np.array_equal(dec[~ok].view(np.uint32), a[~ok].view(np.uint32))
        assert float(np.max(np.abs(dec[ok].astype(np.float64) - a[ok].astype(np.float64)))) <= 1e-3
        h, o, sec = szh_ref.parse(_payload_of(blob))
        assert h["n_vout"] > 0 and (h["n_dout"] > 0 or mask == "R")  # (regression only: no Lorenzo deltas)
        model, _ = szh_ref.reconstruct_blocks(h, sec, szh_ref.huffman_decode(h, sec))
        assert np.array_equal(model.view(np.uint32), dec.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("shape,eb", [((1 << 20,), 1e-3), ((1 << 18,), 2e-2), ((1024, 1024), 1e-3), ((768, 1000), 0.15)],
                         ids=["C1", "1d-coarse", "2d", "2d-coarse"])
def test_ratio_and_selection_against_the_oracle(shape, eb):
    """SURVEY.md 8(d) C1 (the first 2^20 values of the C2 field, ALGO_LORENZO_REG defaults: Lorenzo + regression, blocks of 128,
    abs 1e-3) and a 2-D field, each also at a bound where regression takes a visible share. Bound strict; ratio >= 0.95 x the
    oracle's for the same predictor set; the selection vector against the oracle's own choices block by block."""
    a = _field(shape, np.float32)
    oconf = make_config(a.shape, abs_eb=eb, lorenzo=True, regression=True)
    o_ratio = a.nbytes / len(oracle_compress(a, oconf))
    osel = oracle_selection(a, oconf)
    blob, ratio = sz3_amd.compress(a, _conf(shape, eb, 1, 0, 1))
    dec, c2 = sz3_amd.decompress(blob, np.float32, shape)
    assert float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= eb
    assert (c2.lorenzo, c2.lorenzo2, c2.regression) == (1, 0, 1)
    h, o, sec = szh_ref.parse(_payload_of(blob))
    assert h["predictor"] == 2 and h["ndim"] == len(shape)
    sel = np.asarray(szh_ref.parse_side(h, sec)[0]).reshape(-1)
    assert osel.size == sel.size and (osel >= 0).all()
    same = float((osel == sel).mean())
    print("%s @%g: ratio %.2f (oracle %.2f); regression blocks %.3f (oracle %.3f); selection identical in %.2f %% of the blocks"
          % (shape, eb, ratio, o_ratio, float((sel == 2).mean()), float((osel == 2).mean()), 100 * same))
    assert ratio >= 0.95 * o_ratio
    assert same >= 0.925  # (measured 94.5 - 99.99 %)


def test_full_size_round_trip_of_a_long_series():
    """2^26 values in blocks of 128 (524 288 blocks: the block scan's tiles of 1024 chained 512 times), f64"""
    a = field1d(1 << 22, np.float64)
    a = np.tile(a, 16)
    a += np.repeat(np.arange(16, dtype=np.float64), 1 << 22) * 0.37
    conf = _conf(a.shape, 1e-4, 1, 0, 1)
    blob, ratio = sz3_amd.compress(a, conf)
    dec, c2 = sz3_amd.decompress(blob, np.float64, a.shape)
    assert float(np.max(np.abs(dec - a))) <= 1e-4
    assert (c2.lorenzo, c2.regression) == (1, 1)


@pytest.mark.parametrize("shape,block,eb", [((300, 517), None, 0.15), ((130, 70), 8, 0.15), ((17, 1000), 16, 1e-3), ((64, 64), 16, 0.2), ((1000, 1300), 12, 0.15)])
def test_grouped_and_per_block_2d_decoders_agree(shape, block, eb):
    """2-D blocks of up to 16 x 16 are decoded in groups of 4 x 4 per workgroup, the whole chain of fronts in one launch
    (k_blkn_wave2: tickets in the fronts' order, flags, closed form); Dbg.BLKDEC_PER_FRONT takes round 3's launch per front (inner fronts
    through a shared LDS tile, DPP row scans), Dbg.BLKDEC_BLOCK_PER_WAVE the block-per-wave fronts: same array, bit for bit, with ragged and missing
    blocks in the last groups, on fields where regression blocks sit among the Lorenzo blocks"""
    for dtype in (np.float32, np.float64):
        a = field2d(shape, dtype)
        a[shape[0] // 2:, :] += 3.0
        blob, _ = sz3_amd.compress(a, _conf(shape, eb, 1, 0, 1, block=block))
        outs = []
        # (FORCE_RETRY: the retry a flag poll that gave up takes)
        for flag in (NO_EXIT, NO_EXIT | Dbg.BLKDEC_FORCE_RETRY, NO_EXIT | Dbg.BLKDEC_PER_FRONT, NO_EXIT | Dbg.BLKDEC_BLOCK_PER_WAVE):
            with sz3_amd.debug_flags(flag):
                dec, c2 = sz3_amd.decompress(blob, dtype, shape)
                outs.append(dec)
        assert all(np.array_equal(outs[0], o) for o in outs[1:])
        assert float(np.max(np.abs(outs[0].astype(np.float64) - a.astype(np.float64)))) <= eb
        h, o, sec = szh_ref.parse(_payload_of(blob))
        if h["predictor"] == 2:  # (the selection may hand a field over to the plain path: nothing to compare then)
            sel = np.asarray(szh_ref.parse_side(h, sec)[0])
            print(shape, dtype.__name__, "regression blocks %.3f" % float((sel == 2).mean()))


@pytest.mark.plain_exit
@pytest.mark.parametrize("shape,eb,exits", [((1024, 1024), 1e-3, True), ((1 << 20,), 1e-3, False), ((700, 900), 0.15, False)], ids=["2d", "C1", "2d-coarse"])
def test_low_dimensional_fields_where_only_lorenzo_is_chosen_become_the_plain_stream(shape, eb, exits):
    """as in 3-D: the selection runs first (k_blkn_fit's selection form); fewer than one block in 4096 choosing regression -> the
    array goes to the plain Lorenzo path and the payload IS the one `regression = 0` gives; C1 (18 % regression blocks) keeps
    its block stream. (In 1-D the exit is rare: the estimate looks at a block's two ends only, and a line through 128 values of
    noise above the bound beats the previous value there — as in the reference.)"""
    a = _field(shape, np.float32)
    blob, ratio = sz3_amd.compress(a, _conf(shape, eb, 1, 0, 1))
    dec, c2 = sz3_amd.decompress(blob, np.float32, shape)
    assert float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= eb
    h, o, sec = szh_ref.parse(_payload_of(blob))
    plain, _ = sz3_amd.compress(a, _conf(shape, eb, 1, 0, 0))
    if exits:
        assert h["predictor"] == 0 and (c2.lorenzo, c2.regression) == (1, 0)
        assert _payload_of(blob) == _payload_of(plain)
    else:
        assert h["predictor"] == 2 and (c2.lorenzo, c2.regression) == (1, 1)


@pytest.mark.parametrize("n,block,dtype", [(1 << 20, None, np.float32), (100003, 100, np.float32), (40000, 7, np.float64), (100003, 104, np.float64), (5001, 8, np.float32)])
def test_1d_fit_by_rows_of_lanes_and_by_waves_agree(n, block, dtype):
    """1-D: four blocks per wave (a block per DPP row of 16 lanes, k_blkn_fit_rows) against a wave per block (Dbg.BLK_1D_WAVE_PER_BLOCK):
    the same choices and the same stream (the sums are taken in a different order: coefficients could differ in the last bit of a
    double, not on these fields)"""
    a = field1d(n, dtype)
    conf = _conf((n,), 1e-3, 1, 0, 1, block=block)
    blobs = []
    for flag in (NO_EXIT, NO_EXIT | Dbg.BLK_1D_WAVE_PER_BLOCK):
        with sz3_amd.debug_flags(flag):
            blob, _ = sz3_amd.compress(a, conf)
            blobs.append(_payload_of(blob))
    h0, _, s0 = szh_ref.parse(blobs[0])
    h1, _, s1 = szh_ref.parse(blobs[1])
    sel0, sel1 = np.asarray(szh_ref.parse_side(h0, s0)[0]), np.asarray(szh_ref.parse_side(h1, s1)[0])
    assert np.array_equal(sel0, sel1) and (sel0 == 2).any() and (sel0 == 0).any()
    assert blobs[0] == blobs[1]
    # ... and the decoder's Lorenzo pass: rows of lanes (blocks of up to 128 values, a multiple of 8) against a wave per block
    blob, _ = sz3_amd.compress(a, conf)
    outs = []
    for flag in (0, Dbg.BLK_1D_WAVE_PER_BLOCK):
        with sz3_amd.debug_flags(flag):
            outs.append(sz3_amd.decompress(blob, dtype, (n,))[0])
    assert outs[0].tobytes() == outs[1].tobytes()
    assert float(np.max(np.abs(outs[0].astype(np.float64) - a.astype(np.float64)))) <= 1e-3


@pytest.mark.parametrize("shape", [(1,), (2,), (3,), (5,), (20,), (129,), (257,), (2, 2), (3, 5), (1, 9), (16, 17), (33, 2)])
def test_tiny_and_degenerate_low_dimensional_arrays(shape):
    """arrays of a few values, single ragged blocks, blocks of one row or one value (regression is not valid there:
    RegressionPredictor.hpp:33-36 -> the Lorenzo-1 fallback, BlockwiseDecomposition.hpp:35-37): the bound holds, whatever stream
    the dispatcher's fallbacks choose; both predictor sets"""
    rng = np.random.default_rng(5)
    a = (np.cumsum(rng.normal(size=int(np.prod(shape)))).reshape(shape) * 0.01).astype(np.float32)
    for mask in ("L1+R", "R"):
        conf = _conf(shape, 1e-3, *MASKS[mask])
        blob, _ = sz3_amd.compress(a, conf)
        dec, c2 = sz3_amd.decompress(blob, np.float32, shape)
        assert dec.shape == a.shape and float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= 1e-3


# ---- second-order Lorenzo in 1-D (round 4: k_blkn2_*, the scan of affine maps) ----------------------------------------------
# LorenzoPredictor.hpp:69-71 (2 d[-1] - d[-2]), noise 1.08 eb (:17-38); the set [Lorenzo-1, Lorenzo-2] with blocks of 128 is what the
# reference's default algorithm compresses a 1-D array with whenever its sampling test prefers Lorenzo (SZAlgoInterp.hpp:232-282).
L2_MASKS = ["L2", "L1+L2", "L1+L2+R", "L2+R"]


@pytest.mark.parametrize("mask", L2_MASKS)
@pytest.mark.parametrize("dtype,n,eb,block", [(np.float32, 5000, 1e-3, None), (np.float64, 3001, 2e-2, 64), (np.float32, 130, 1e-2, 7),
                                             (np.float32, 100003, 1e-4, 5), (np.float64, 2500, 1e-5, 1000), (np.float64, 40001, 1e-4, 104),
                                             (np.float32, 5001, 1e-3, 8)])
def test_1d_second_order_block_stream_against_the_numpy_model(mask, dtype, n, eb, block):
    a = field1d(n, dtype)
    conf = _conf((n,), eb, *MASKS[mask], block=block)
    blob, ratio = sz3_amd.compress(a, conf)
    dec, c2 = sz3_amd.decompress(blob, dtype, (n,))
    assert float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= eb
    if c2.cmprAlgo == sz3_amd.ALGO_LOSSLESS:
        pytest.skip("tiny field went lossless")
    h, o, sec = szh_ref.parse(_payload_of(blob))
    assert h["predictor"] == 2 and h["ndim"] == 1 and h["blk_edge"] == (block or 128)
    assert h["blk_mask"] == sum(b << i for i, b in enumerate(MASKS[mask]))
    assert (c2.lorenzo, c2.lorenzo2, c2.regression) == MASKS[mask]
    codes = szh_ref.huffman_decode(h, sec)
    model, sel = szh_ref.reconstruct_blocks(h, sec, codes)
    assert np.array_equal(model, dec), "numpy model of the block decoder and the GPU decoder disagree"
    sel = np.asarray(sel).reshape(-1)
    allowed = {i for i, b in enumerate(MASKS[mask]) if b} | {0}  # (0: the fallback of a regression that is not valid)
    assert set(np.unique(sel)) <= allowed
    print(n, mask, "ratio %.2f" % ratio, "shares L1 %.3f L2 %.3f R %.3f" % tuple(float((sel == k).mean()) for k in range(3)))
    # sets of Lorenzo members only take a pass of their own for the choices (k_blkn_sel12) and code straight from the array;
    # Dbg.BLK_1D_WAVE_PER_BLOCK sends them through the general fit pass (q~ of every element through the work array): same stream
    try:
        sz3_amd.lib().sz3hip_debug_flags(NO_EXIT | Dbg.BLK_1D_WAVE_PER_BLOCK)
        blob2, _ = sz3_amd.compress(a, conf)
    finally:
        sz3_amd.lib().sz3hip_debug_flags(NO_EXIT)
    assert _payload_of(blob2) == _payload_of(blob)
    # ... and the decoder by rows of lanes (blocks of up to 128 values, a multiple of 8) against a wave per block: the same array
    try:
        sz3_amd.lib().sz3hip_debug_flags(NO_EXIT | Dbg.BLK_1D_WAVE_PER_BLOCK)
        dec2, _ = sz3_amd.decompress(blob, dtype, (n,))
    finally:
        sz3_amd.lib().sz3hip_debug_flags(NO_EXIT)
    assert dec2.tobytes() == dec.tobytes()


@pytest.mark.parametrize("n,eb,mask", [(1 << 20, 1e-3, "L1+L2"), (1 << 20, 1e-4, "L1+L2"), (1 << 18, 1e-2, "L1+L2"), (1 << 19, 1e-3, "L1+L2+R"), (1 << 18, 1e-3, "L2")])
def test_1d_second_order_ratio_and_selection_against_the_oracle(n, eb, mask):
    """the set the reference's tuner chooses in 1-D (Lorenzo-1 + Lorenzo-2, blocks of 128) on the C1 field, and the sets around it:
    bound strict, ratio >= 0.95 x the oracle's, the choices block by block (on C1 at 1e-3 second-order blocks are what lifts the
    oracle's ratio from 5.6 to 7.3)"""
    a = field1d(n, np.float32)
    l1, l2, r = MASKS[mask]
    oconf = make_config(a.shape, abs_eb=eb, lorenzo=bool(l1), lorenzo2=bool(l2), regression=bool(r))
    o_ratio = a.nbytes / len(oracle_compress(a, oconf))
    osel = oracle_selection(a, oconf)
    blob, ratio = sz3_amd.compress(a, _conf((n,), eb, l1, l2, r))
    dec, c2 = sz3_amd.decompress(blob, np.float32, (n,))
    assert float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= eb
    assert (c2.lorenzo, c2.lorenzo2, c2.regression) == (l1, l2, r)
    h, o, sec = szh_ref.parse(_payload_of(blob))
    assert h["predictor"] == 2 and h["ndim"] == 1
    sel = np.asarray(szh_ref.parse_side(h, sec)[0]).reshape(-1)
    assert osel.size == sel.size and (osel >= 0).all()
    same = float((osel == sel).mean())
    print("1-D %d @%g %s: ratio %.2f (oracle %.2f); second-order blocks %.3f (oracle %.3f); selection identical in %.2f %% of the blocks"
          % (n, eb, mask, ratio, o_ratio, float((sel == 1).mean()), float((osel == 1).mean()), 100 * same))
    assert ratio >= 0.95 * o_ratio
    assert same >= 0.9


def test_1d_second_order_unpredictable_values_wide_deltas_and_long_series():
    a = field1d(40000, np.float32)
    a[5] = np.nan
    a[1234] = np.inf
    a[2000:2300] += 500.0
    for mask in ("L1+L2", "L2", "L1+L2+R"):
        conf = _conf(a.shape, 1e-3, *MASKS[mask])
        conf.quantbinCnt = 1024
        blob, _ = sz3_amd.compress(a, conf)
        dec, _ = sz3_amd.decompress(blob, np.float32, a.shape)
        ok = np.isfinite(a)
        assert np.array_equal(dec[~ok].view(np.uint32), a[~ok].view(np.uint32))
        assert float(np.max(np.abs(dec[ok].astype(np.float64) - a[ok].astype(np.float64)))) <= 1e-3
        h, o, sec = szh_ref.parse(_payload_of(blob))
        assert h["n_vout"] > 0 and h["n_dout"] > 0
        model, _ = szh_ref.reconstruct_blocks(h, sec, szh_ref.huffman_decode(h, sec))
        assert np.array_equal(model.view(np.uint32), dec.reshape(-1).view(np.uint32))
    # 2^24 values in blocks of 128 (131 072 blocks: 128 tiles of the scan), f64, and blocks of 5 (the tuner's trial geometry: 3.4 M blocks)
    b = np.tile(field1d(1 << 22, np.float64), 4)
    b += np.repeat(np.arange(4, dtype=np.float64), 1 << 22) * 0.37
    for block in (None, 5):
        blob, ratio = sz3_amd.compress(b, _conf(b.shape, 1e-4, 1, 1, 0, block=block))
        dec, c2 = sz3_amd.decompress(blob, np.float64, b.shape)
        assert float(np.max(np.abs(dec - b))) <= 1e-4 and (c2.lorenzo, c2.lorenzo2, c2.regression) == (1, 1, 0)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 20, 129, 257])
def test_1d_second_order_tiny_arrays(n):
    rng = np.random.default_rng(5)
    a = (np.cumsum(rng.normal(size=n)) * 0.01).astype(np.float32)
    for mask in L2_MASKS:
        blob, _ = sz3_amd.compress(a, _conf((n,), 1e-3, *MASKS[mask]))
        dec, c2 = sz3_amd.decompress(blob, np.float32, (n,))
        assert dec.shape == a.shape and float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= 1e-3


# ---- second-order Lorenzo in 2-D (round 4: k_blkn_decode2s; LorenzoPredictor.hpp:75-79, noise 2.76 eb) -------------------------------
@pytest.mark.parametrize("mask", L2_MASKS)
@pytest.mark.parametrize("dtype,shape,eb,block", [(np.float32, (70, 90), 1e-2, None), (np.float64, (33, 47), 2e-2, 8), (np.float32, (64, 96), 5e-2, 32),
                                                 (np.float32, (5, 200), 1e-3, 4), (np.float32, (130, 131), 1e-4, 16)])
def test_2d_second_order_block_stream_against_the_numpy_model(mask, dtype, shape, eb, block):
    a = field2d(shape, dtype)
    conf = _conf(shape, eb, *MASKS[mask], block=block)
    blob, ratio = sz3_amd.compress(a, conf)
    dec, c2 = sz3_amd.decompress(blob, dtype, shape)
    assert float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= eb
    if c2.cmprAlgo == sz3_amd.ALGO_LOSSLESS:
        pytest.skip("tiny field went lossless")
    h, o, sec = szh_ref.parse(_payload_of(blob))
    assert h["predictor"] == 2 and h["ndim"] == 2 and h["blk_edge"] == (block or 16)
    assert h["blk_mask"] == sum(b << i for i, b in enumerate(MASKS[mask]))
    assert (c2.lorenzo, c2.lorenzo2, c2.regression) == MASKS[mask]
    codes = szh_ref.huffman_decode(h, sec)
    model, sel = szh_ref.reconstruct_blocks(h, sec, codes)
    assert np.array_equal(model.reshape(shape), dec), "numpy model of the block decoder and the GPU decoder disagree"
    sel = np.asarray(sel).reshape(-1)
    print(shape, mask, "ratio %.2f" % ratio, "shares L1 %.3f L2 %.3f R %.3f" % tuple(float((sel == k).mean()) for k in range(3)))
    # the encoder without the selection pass in front (the fit pass chooses, q~ of every element through the work array): same stream
    try:
        sz3_amd.lib().sz3hip_debug_flags(NO_EXIT | Dbg.BLK_NO_SELECT)
        blob2, _ = sz3_amd.compress(a, conf)
    finally:
        sz3_amd.lib().sz3hip_debug_flags(NO_EXIT)
    assert _payload_of(blob2) == _payload_of(blob)


@pytest.mark.parametrize("shape,eb,mask", [((1024, 1024), 1e-3, "L1+L2"), ((768, 1000), 1e-4, "L1+L2"), ((512, 640), 0.15, "L1+L2+R"), ((600, 700), 1e-2, "L2")])
def test_2d_second_order_ratio_and_selection_against_the_oracle(shape, eb, mask):
    a = field2d(shape, np.float32)
    l1, l2, r = MASKS[mask]
    oconf = make_config(a.shape, abs_eb=eb, lorenzo=bool(l1), lorenzo2=bool(l2), regression=bool(r))
    o_ratio = a.nbytes / len(oracle_compress(a, oconf))
    osel = oracle_selection(a, oconf)
    blob, ratio = sz3_amd.compress(a, _conf(shape, eb, l1, l2, r))
    dec, c2 = sz3_amd.decompress(blob, np.float32, shape)
    assert float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= eb
    h, o, sec = szh_ref.parse(_payload_of(blob))
    if h["predictor"] != 2:  # (next to every block chose Lorenzo-1: the plain stream)
        print("2-D %s @%g %s: plain stream, ratio %.2f (oracle %.2f), oracle's second-order share %.4f" % (shape, eb, mask, ratio, o_ratio, float((osel == 1).mean())))
        assert ratio >= 0.95 * o_ratio and float((osel != 0).mean()) < 0.01
        return
    assert (c2.lorenzo, c2.lorenzo2, c2.regression) == (l1, l2, r)
    sel = np.asarray(szh_ref.parse_side(h, sec)[0]).reshape(-1)
    same = float((osel == sel).mean())
    print("2-D %s @%g %s: ratio %.2f (oracle %.2f); second-order blocks %.3f (oracle %.3f); selection identical in %.2f %% of the blocks"
          % (shape, eb, mask, ratio, o_ratio, float((sel == 1).mean()), float((osel == 1).mean()), 100 * same))
    assert ratio >= 0.95 * o_ratio
    assert same >= 0.9
