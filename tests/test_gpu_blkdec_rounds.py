"""GPU tests (-m gpu) of the block decoders past their first round (sz3hip_regress.hip; DESIGN.md, "The block decoders past their
first round"): the one-launch decoders k_blkn_wave2 (2-D) and k_blk_wave3 (3-D) on arrays with more groups than the launch has
workgroups, so that a workgroup takes a second ticket on an LDS tile that still holds its previous group, and the 1-D top scans
k_blkn_scan_top / k_blkn2_top over more than 1024 tiles, so that their loop takes a second step with the carried inflow.

Each case compresses once and decodes under the default flags and under every launch-per-front form: all outputs byte for byte the
same, the default one byte for byte the numpy model's (szh_ref.reconstruct_blocks of the parsed stream), bound and NaN bits kept. What
the decoder did is read from sz3_amd.debug_blkdec_last(): the expected form ran, no retry, and more slots than workgroups / more than
1024 tiles — if the caps in blk_decompress_impl change, these assertions fail instead of the cases going quiet.

The shapes are the smallest that reach the second round: groups of 4 x 4 blocks (2-D) against 2048 (f32) / 1024 (f64) workgroups,
groups of 3 x 3 x 3 blocks of 6^3 (3-D) against 1024 / 512, tiles of 1024 blocks (1-D) against the 1024 threads of the top scan.

Measured on one MI355X (regression share of the blocks; seconds for the model / for the whole case; the 23 tests took 19 s):
    2-D (725, 717) B 4 f32 0.626 (0.3 / 1.3)     (1283, 1257) B 7 f32 0.340 (0.5 / 0.8)    (520, 505) B 4 f64 0.630 (0.1 / 0.4)
        (2060, 2000) B 16 f64 0.417 (0.3 / 0.8)  (20, 33603) B 4 f32 and f64 0.568 (0.3 / 0.4)
    3-D (150, 130, 140) f64 0.113 (0.2 / 0.4)    (185, 170, 165) f32 0.120 (0.3 / 0.9)     (7, 20, 10805) f32 and f64 0.240 (0.2 / 0.4)
    1-D (4200307,) B 4 0.800, with Lorenzo-2 in the set 0.781 beside 0.019 second-order blocks (1.1 / 1.6)
        (8400613,) B 8 0.795, with Lorenzo-2 in the set 0.790 beside 0.118 (2.1 / 2.7)
Every case lists deltas (2 .. 210 000) and values (3 .. 33).
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sz3_amd  # noqa: E402
import szh_ref  # noqa: E402
from fields import field1d, field2d, field3d  # noqa: E402
from test_gpu_regression import MASKS, NO_EXIT, Dbg, _block_streams_wanted, _conf, _payload_of  # noqa: E402,F401  (the autouse fixture: block streams wanted)

Form = sz3_amd.BlkDecForm
TILE = 1024  # blocks per tile of the 1-D scans, and tiles per step of the top scan's loop


def _plant(a, B, step_axis=0):
    """the step the block tests add (+3 on the high half along an axis), a box of +500 whose faces cut through blocks (Lorenzo deltas
    beyond the radius of 512 next to it), a few NaN"""
    sl = [slice(None)] * a.ndim
    sl[step_axis] = slice(a.shape[step_axis] // 2, None)
    a[tuple(sl)] += 3.0
    lo = [min(B + B // 2, d // 2) for d in a.shape]
    a[tuple(slice(l, min(l + 2 * B, d)) for l, d in zip(lo, a.shape))] += 500.0
    flat = a.reshape(-1)
    for i in (5, a.size // 3, a.size - 7):
        flat[i] = np.nan
    return a


def _field_1d(n, dtype, B):
    """C1 with the existing tests' step (+500 on 300 values, its ends inside blocks). Blocks of 4 or 8 values of this field all but
    always choose regression (a line through so few values beats the previous value at the block's two ends, which is where the
    estimate looks), so the last fifth of the series, which holds the first block of tile 1024, also carries a square wave of period
    2 B that jumps in the middle of every block and is flat across the blocks' ends: there Lorenzo wins, and its blocks are open"""
    a = field1d(n, dtype)
    a[2002:2302] += 500.0
    w0 = (int(0.8 * n) // (2 * B)) * 2 * B
    i = np.arange(w0, n)
    a[w0:] += (3.0 * (((i + B // 2) // B) % 2)).astype(dtype)
    for i in (5, n // 3, TILE * TILE * B + 1, n - 7):
        a[i] = np.nan
    return a


def _decode_all(a, conf, flags):
    """one stream -> ([(flag, output, read-out)], parsed stream)"""
    blob, _ = sz3_amd.compress(a, conf)
    got = []
    for flag in flags:
        with sz3_amd.debug_flags(NO_EXIT | flag):
            dec, _ = sz3_amd.decompress(blob, a.dtype, a.shape)
            got.append((flag, dec, sz3_amd.debug_blkdec_last()))
    return got, szh_ref.parse(_payload_of(blob))


def _check(a, eb, mask, got, parsed, t0):
    """what every case asserts but the read-out: the inputs exercise what the case is about, every form gives the same bytes, the
    model gives them too, bound and NaN bits"""
    h, o, sec = parsed
    assert h["predictor"] == 2 and h["blk_mask"] == sum(b << i for i, b in enumerate(MASKS[mask]))
    sel, coef = szh_ref.parse_side_groups(h, sec)
    share = [float((sel == k).mean()) for k in range(3)]
    default = got[0][1]
    for flag, dec, info in got[1:]:
        assert dec.tobytes() == default.tobytes(), "decoder form under flag %d (%s) differs from the default form" % (int(flag), info["form"].name)
    ok = np.isfinite(a)
    U = np.uint32 if a.dtype == np.float32 else np.uint64
    assert not ok.all() and np.array_equal(default[~ok].view(U), a[~ok].view(U)), "NaN bits"
    assert float(np.max(np.abs(default[ok].astype(np.float64) - a[ok].astype(np.float64)))) <= eb
    t1 = time.time()
    model, _ = szh_ref.reconstruct_blocks(h, sec, szh_ref.huffman_decode_units(h, sec), side=(sel, coef))
    t2 = time.time()
    print("%s %s B %d %s @%g: shares L1 %.3f L2 %.3f R %.3f; listed deltas %d, listed values %d; model %.1f s, case %.1f s; %s"
          % (a.shape, a.dtype.name, h["blk_edge"], mask, eb, *share, h["n_dout"], h["n_vout"], t2 - t1, t2 - t0,
             {k: (v.name if isinstance(v, Form) else int(v)) for k, v in got[0][2].items()}))
    assert model.tobytes() == default.tobytes(), "numpy model of the block decoder and the GPU decoder disagree"
    assert 0.05 <= share[2] <= 0.95, "Lorenzo and regression blocks must share groups"
    assert h["n_vout"] > 0 and h["n_dout"] > 0
    return sel


def _check_one_launch(got, form, retry_form, nslots, cap, others):
    for flag, dec, info in got:
        if flag in (0, Dbg.BLKDEC_FORCE_RETRY, Dbg.BLKDEC_LOCAL_EXPANDED):
            assert info["form"] == form and info["nslots"] == nslots and info["workgroups"] == cap, info
            assert info["nslots"] > info["workgroups"] > 0, "no workgroup takes a second ticket: %r" % info
            assert info["retried"] == (flag == Dbg.BLKDEC_FORCE_RETRY), info  # (default flags: no flag poll gave up)
            assert info["retry_form"] == (retry_form if flag == Dbg.BLKDEC_FORCE_RETRY else Form.NONE), info
        else:
            assert info["form"] in others[flag] and not info["retried"] and info["workgroups"] == 0, info


FLAGS_2D = (0, Dbg.BLKDEC_FORCE_RETRY, Dbg.BLKDEC_PER_FRONT, Dbg.BLKDEC_BLOCK_PER_WAVE)
FLAGS_3D = FLAGS_2D + (Dbg.BLKDEC_GROUPS_3, Dbg.BLKDEC_LOCAL_EXPANDED)
FLAGS_1D = (0, Dbg.BLK_1D_WAVE_PER_BLOCK)


@pytest.mark.parametrize("dtype,shape,block,eb,slots", [
    (np.float32, (725, 717), 4, 1e-2, 46 * 45), (np.float32, (1283, 1257), 7, 3e-2, 46 * 45),
    (np.float64, (520, 505), 4, 1e-2, 33 * 32), (np.float64, (2060, 2000), None, 0.15, 33 * 32),
    (np.float32, (20, 33603), 4, 1e-2, 2 * 2101), (np.float64, (20, 33603), 4, 1e-2, 2 * 2101)],
    ids=["f32-B4", "f32-B7", "f64-B4", "f64-B16", "f32-thin", "f64-thin"])
def test_2d_one_launch_decoder_takes_second_tickets(dtype, shape, block, eb, slots):
    """k_blkn_wave2: ragged last groups in both directions; the thin shape has fronts of at most two groups, so a workgroup's second
    ticket lies some 1000 (f32) / 500 (f64) fronts behind its first"""
    t0 = time.time()
    a = _plant(field2d(shape, dtype), block or 16)
    conf = _conf(shape, eb, *MASKS["L1+R"], block=block)
    conf.quantbinCnt = 1024
    got, parsed = _decode_all(a, conf, FLAGS_2D)
    _check_one_launch(got, Form.WAVE_2D, Form.GROUPS_2D, slots, 2048 if dtype == np.float32 else 1024,
                      {Dbg.BLKDEC_PER_FRONT: (Form.GROUPS_2D,), Dbg.BLKDEC_BLOCK_PER_WAVE: (Form.FRONTS_2D,)})
    _check(a, eb, "L1+R", got, parsed, t0)


@pytest.mark.parametrize("dtype,shape,mask,eb,step_axis,slots", [
    (np.float64, (150, 130, 140), "L1+R", 3e-2, 0, 9 * 8 * 8), (np.float64, (150, 130, 140), "L1+L2+R", 3e-2, 0, 9 * 8 * 8),
    (np.float32, (185, 170, 165), "L1+R", 3e-2, 0, 11 * 10 * 10), (np.float32, (185, 170, 165), "L1+L2+R", 3e-2, 0, 11 * 10 * 10),
    (np.float32, (7, 20, 10805), "L1+R", 5e-2, 2, 1 * 2 * 601), (np.float64, (7, 20, 10805), "L1+R", 5e-2, 2, 1 * 2 * 601)],
    ids=["f64-L1R", "f64-L1L2R", "f32-L1R", "f32-L1L2R", "f32-chain", "f64-chain"])
def test_3d_one_launch_decoder_takes_second_tickets(dtype, shape, mask, eb, step_axis, slots):
    """k_blk_wave3: ragged and missing blocks in the last groups; the thin shape is a chain of some 600 fronts of at most two groups
    (its step lies along x: with 7 planes a step along z would leave no block to regression)"""
    t0 = time.time()
    a = _plant(field3d(shape, dtype), 6, step_axis)
    conf = _conf(shape, eb, *MASKS[mask])
    conf.quantbinCnt = 1024
    got, parsed = _decode_all(a, conf, FLAGS_3D)
    per_front = (Form.GROUPS_2_3D,) if sz3_amd.lib().sz3hip_lab_build() else (Form.FRONTS_3D,)
    _check_one_launch(got, Form.WAVE_3D, Form.GROUPS_3_3D, slots, 1024 if dtype == np.float32 else 512,
                      {Dbg.BLKDEC_PER_FRONT: per_front, Dbg.BLKDEC_BLOCK_PER_WAVE: (Form.FRONTS_3D,), Dbg.BLKDEC_GROUPS_3: (Form.GROUPS_3_3D,)})
    _check(a, eb, mask, got, parsed, t0)


@pytest.mark.parametrize("mask", ["L1+R", "L1+L2+R"])
@pytest.mark.parametrize("dtype,n,block,eb", [(np.float32, 4200307, 4, 1e-3), (np.float64, 4200307, 4, 1e-3), (np.float32, 8400613, 8, 3e-2)],
                         ids=["f32-B4", "f64-B4", "f32-B8"])
def test_1d_top_scan_takes_a_second_step(mask, dtype, n, block, eb):
    """k_blkn_scan_top (L1+R) / k_blkn2_top (L1+L2+R) over 1026 tiles: blocks of 4 go a wave per block, blocks of 8 four per wave.
    The first block of tile 1024 is a Lorenzo block: it is open and takes the inflow the loop carried into its second step"""
    t0 = time.time()
    a = _field_1d(n, dtype, block)
    conf = _conf((n,), eb, *MASKS[mask], block=block)
    conf.quantbinCnt = 1024
    got, parsed = _decode_all(a, conf, FLAGS_1D)
    tiles = ((n + block - 1) // block + TILE - 1) // TILE
    for flag, dec, info in got:
        assert info["form"] == (Form.SCAN2_1D if mask == "L1+L2+R" else Form.SCAN_1D) and not info["retried"] and info["workgroups"] == 0, info
        assert info["tiles"] == tiles and info["tiles"] > TILE, "the top scan's loop takes one step only: %r" % info
        assert info["rows"] == (block % 8 == 0 and flag == 0), info
    sel = _check(a, eb, mask, got, parsed, t0).reshape(-1)
    assert sel[TILE * TILE] != 2, "the first block of tile 1024 must be a Lorenzo block"
