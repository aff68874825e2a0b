"""GPU tests (-m gpu): the randomised sweeps of tests/checks/ as part of the suite (fixed seeds, a few seconds each).
tests/checks/lorenzo_sweep.py  - K1 codes / outlier counts / payload decode against the numpy model of the format (tests/szh_ref.py)
tests/checks/interp_sweep.py   - interpolation codes and reconstruction against the oracle, bit for bit
tests/checks/host_sweep.py     - the host API over dtypes, error-bound modes and algorithms: the user-visible guarantee of each mode
tests/checks/block_sweep.py    - the block-composed path (predictor sets, block edges, radii, NaNs, steps) against the numpy block decoder
They found the small-quantbinCnt bugs fixed in round 1 (code 0 inside the kernels' LDS histogram windows)."""
import os
import subprocess
import sys

import pytest

import sz3_amd
from sweep_seeds import (DEVICE_VIEW_SWEEP_N, DEVICE_VIEW_SWEEP_SEEDS, PARTIAL_SWEEP_N, PARTIAL_SWEEP_SEEDS, SAMPLED_SWEEP_N, SAMPLED_SWEEP_SEEDS,
                         WIDEBOOK_SWEEP_N, WIDEBOOK_SWEEP_SEEDS)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tool, seed, n, flags=None):
    env = dict(os.environ, SEED=str(seed), N=str(n))
    if flags is not None:
        env["DBG_FLAGS"] = str(int(flags))  # (the checks read a number)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", tool)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("seed", [11, 12])
def test_lorenzo_sweep(seed):
    out = _run("lorenzo_sweep.py", seed, 30)
    assert "mismatches: 0" in out, out[-3000:]


@pytest.mark.parametrize("seed", [11, 12])
def test_interp_sweep(seed):
    out = _run("interp_sweep.py", seed, 25)
    assert "mismatches: 0" in out, out[-3000:]


def test_interp_sweep_through_the_level_kernels():
    """Dbg.INTERP_LEVELS_ANY_SIZE: every level of every 3-D case runs in the level kernels (the sweep's arrays are below their size)"""
    out = _run("interp_sweep.py", 13, 40, flags=sz3_amd.Dbg.INTERP_LEVELS_ANY_SIZE)
    assert "mismatches: 0" in out, out[-3000:]


@pytest.mark.parametrize("seed", [1, 2])
def test_block_path_sweep(seed):
    out = _run("block_sweep.py", seed, 30)
    assert "mismatches: 0" in out, out[-3000:]


@pytest.mark.parametrize("ndim,n", [(1, 30), (2, 30), (4, 16)])
def test_block_path_sweep_in_other_dimensions(ndim, n, monkeypatch):
    """the same sweep over 1-D, 2-D (every set, second-order Lorenzo included: round 4) and 4-D arrays (Lorenzo-1 / regression)"""
    monkeypatch.setenv("NDIM", str(ndim))
    out = _run("block_sweep.py", 5, n)
    assert "mismatches: 0" in out, out[-3000:]


def test_host_api_sweep():
    out = _run("host_sweep.py", 11, 40)
    assert "failures: 0" in out, out[-3000:]


BIG = [  # (id, algorithm, shape, dtype, abs bound, noise, GiB of free HBM needed)
    ("4.4e9-f32-lorenzo", "lorenzo", "1100,2000,2000", "f32", "1e-3", "2e-3", 120),
    ("4.4e9-f32-interp", "interp", "1100,2000,2000", "f32", "1e-3", "2e-3", 120),
    ("C5-whole-lorenzo", "lorenzo", "100,500,500,500", "f32", "2.4e-3", "2e-3", 225),
    ("C5-whole-default-REL1e-3", "default", "100,500,500,500", "f32", "rel:1e-3", "2e-3", 225),  # (BASELINE.json configs[4]: REL errBound through the device range scan)
    ("C4-whole-lorenzo", "lorenzo", "1024,1024,1024", "f64", "1e-6", "2e-6", 60),
    ("C4-whole-default", "default", "1024,1024,1024", "f64", "1e-6", "2e-6", 60),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BIG, ids=[c[0] for c in BIG])
def test_round_trip_at_full_benchmark_sizes_and_beyond_2_pow_32_elements(case):
    """BASELINE.json's largest configurations whole on ONE GPU - C5 100 x 500^3 f32 (1.25e10 elements, 50 GB) and C4 1024^3 f64
    (8 GiB) - and 1100 x 2000 x 2000 f32 (4.4e9 elements): every index, chunk and list position beyond 32 bits. The field is
    generated and the error bound checked slab by slab on the device (tests/checks/big_roundtrip.py, a process of its own)"""
    import torch
    _, algo, shape, dtype, eb, sigma, need = case
    import time
    for _ in range(30):  # (the previous case's process has exited, the driver may still be handing its memory back)
        free, _ = torch.cuda.mem_get_info(0)
        if free >= need * 2 ** 30:
            break
        time.sleep(1.0)
    if free < need * 2 ** 30:
        pytest.skip("needs %d GiB of free HBM, %.0f free" % (need, free / 2 ** 30))
    n = 1
    for d in shape.split(","):
        n *= int(d)
    env = dict(os.environ, LAB_ALGO=algo, LAB_SHAPE=shape, LAB_EB=eb, LAB_DTYPE=dtype, LAB_SIGMA=sigma)
    if eb.startswith("rel:"):
        env.update(LAB_REL=eb[4:], LAB_EB="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "big_roundtrip.py")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " OK " in last and str(n) in r.stdout, last


@pytest.mark.parametrize("seed", [11, 12])
def test_exact_tuner_sweep(seed):
    """tests/checks/tuner_exact_sweep.py: 25 random arrays (1-D .. 4-D, f32 / f64, smooth / noisy, bounds over four decades) — with the
    trials priced the reference's way every interpolation trial's compressed size equals the reference's byte for byte and every decision
    (linear / cubic, order, (alpha, beta), interpolation or Lorenzo, the Lorenzo quantizer) is the reference's"""
    out = _run("tuner_exact_sweep.py", seed, 25)
    assert "mismatches 0" in out


@pytest.mark.parametrize("seed", [21, 22])
def test_stock_containers_sweep(seed):
    """tests/checks/stock_bytes_sweep.py: 40 random calls in stock format (ALGO_INTERP with random parameters, the default algorithm, Lorenzo sets
    of one member, mixed sets in every dimension since round 6; 1-D .. 4-D, f32 / f64, absolute and relative bounds) — every container is the reference's, byte for byte"""
    out = _run("stock_bytes_sweep.py", seed, 40)
    assert "mismatches 0" in out


@pytest.mark.parametrize("seed", [31, 32])
def test_default_algorithm_reconstruction_sweep(seed):
    """tests/checks/default_algo_recon_sweep.py: 25 random 2-D .. 4-D arrays under the reference's default algorithm through the host API, this
    library's own stream format — decompressed bit for bit to what the reference's stream decompresses to"""
    out = _run("default_algo_recon_sweep.py", seed, 25)
    assert "mismatches 0" in out



@pytest.mark.parametrize("seed", [41, 42])
def test_context_history_sweep(seed):
    """tests/checks/history_sweep.py (round 6): one device context through 60 random calls (predictor sets, bounds, shapes up to 4 M elements
    — the sampled book's path —, speculation switched, decompressions in between) against a fresh context on every call: the payload is a
    function of the input and the configuration, whatever the context did before"""
    out = _run("history_sweep.py", seed, 60)
    assert "mismatches 0" in out


@pytest.mark.parametrize("seed", [51, 52])
def test_wild_data_sweep(seed):
    """tests/checks/wild_data_sweep.py (round 6): 60 arrays of the kinds the other sweeps do not draw — white noise, constants, zeros, steps, spikes
    of 1e30, bounds below the values' spacing, magnitudes of 1e30 and f32 denormals, integer-valued floats, negative zeros, NaN / Inf — under a
    random algorithm: this library's payload within the bound; in stock format the container's bytes are the reference's (given the reference's
    capacity: its rule for giving a lossy stream up is about the caller's buffer), and the reference's container reads back to the reference's own
    values bit for bit. (Not counted: non-finite values under a set with the regression member — NaN coefficients' signs, containers the reference
    cannot read back itself.)"""
    out = _run("wild_data_sweep.py", seed, 60)
    assert "failures 0" in out


def test_integer_wild_sweep():
    """tests/checks/int_wild_sweep.py (round 6): 60 integer arrays over all eight integer types — the full range of the type, constants, steps,
    alternating extremes, magnitudes beyond 2^53, bounds from 0.4 (lossless) to 1e6, every algorithm: dtype and shape kept, |x - x^| <= floor(eb)"""
    out = _run("int_wild_sweep.py", 61, 60)
    assert "failures: 0" in out


def test_context_history_sweep_with_wild_arrays(monkeypatch):
    """the same with noise, constants, zeros, spikes of 1e30, steps and bounds near the values' spacing among the calls (WILD=1): calls the lists
    cannot hold end in SZ3HIP_EOUTLIERS and the context goes on — the next payloads are a fresh context's"""
    monkeypatch.setenv("WILD", "1")
    out = _run("history_sweep.py", 43, 120)
    assert "mismatches 0" in out


@pytest.mark.parametrize("seed", PARTIAL_SWEEP_SEEDS)
def test_partial_decode_sweep(seed):
    """tests/checks/partial_sweep.py: 15 random cases of the partial decodes per seed — ranks 1 .. 4 at edge extents, every
    interpolation order, anchor strides 0 .. 64 and the default, raw records and non-finite values in the field, boxes of mixed levels on every
    route (chain, merged sequence, level group by level group) — through the region / tile / tiles / coarse calls, Stream.request into arrays,
    atlas rectangles and stepped views, and two of the five sinks, byte for byte against this library's full decode, a device context's, or the
    ORACLE's decode of a container the oracle wrote. The same seeds pass the plan functions and the coverage floors in
    test_partial_sweep_cpu.py; at most one in ten interpolation cases may open as a fallback handle."""
    out = _run("partial_sweep.py", seed, PARTIAL_SWEEP_N)
    assert "failures 0" in out, out[-3000:]


@pytest.mark.parametrize("seed", SAMPLED_SWEEP_SEEDS)
def test_sampled_path_sweep(seed):
    """tests/checks/sampled_sweep.py: per seed four drawn arrays and two fixed ones of 2^22 .. 6.5e6 elements on the
    sampled-book Lorenzo path — ranks 1 .. 3 at the extents where stage 1's tasks end ragged, f32 and f64, eight kinds of data, neighbours that
    must not take the path — the first payload held to the numpy model in full (codes, lists, header, the book against the sample's counts, the
    chunk table, the slow decoder on up to nine chunks, the decode bit for bit), then the context's later calls, three encoder settings, the
    context after another array and a decoder form byte for byte. The same seeds pass the model's premises and the coverage floors in
    test_sampled_sweep_cpu.py."""
    out = _run("sampled_sweep.py", seed, SAMPLED_SWEEP_N)
    assert "failures 0" in out, out[-3000:]


@pytest.mark.parametrize("seed", WIDEBOOK_SWEEP_SEEDS)
def test_wide_book_sweep(seed):
    """tests/checks/widebook_sweep.py: per seed six drawn histograms of 300 .. 65 535 symbols — flat, geometric, Zipf, a head
    over a rare tail for either tier, Fibonacci tails deeper than the 24- and the 16-bit limit, half of them at a boundary of the three code-book
    constructions — as arrays of 50 K .. 1.5 M elements whose code stream has exactly those counts: the first payload held to the numpy model in
    full (codes, header, the book against widebook_model's tier rule, class weight, Kraft sum and exact optimum, the chunk table, the slow decoder
    on the picked chunks, the decode bit for bit), then the context's second call, one encoder form and one decoder form byte for byte. The same
    seeds pass the model's premises and the coverage floors in test_widebook_sweep_cpu.py."""
    out = _run("widebook_sweep.py", seed, WIDEBOOK_SWEEP_N)
    assert "failures 0" in out, out[-3000:]


@pytest.mark.parametrize("seed", DEVICE_VIEW_SWEEP_SEEDS)
def test_device_view_sweep(seed):
    """tests/checks/device_view_sweep.py: per seed 24 drawn cases of the device-memory calls — the ten element types, ranks
    1 .. 4 at the row walker's inner extents, an input view and another output view (sub-ranges, steps of 2 and 3, permuted memory orders, stride-0
    axes, interleaved fields, bases misaligned or in whole 8- / 16-byte units), every algorithm, the bound modes, stock format, conf.openmp slabs
    and pipelined pieces, non-finite values and integers at their type's ends: the gather hook against numpy's view, the view's container against
    its contiguous copy's and the host API's, the input untouched, the decode's whole allocation against the host decode scattered by numpy, the
    mode's bound, and the coarse call into a drawn view. The same seeds pass their premises and the coverage floors in
    test_device_view_sweep_cpu.py."""
    out = _run("device_view_sweep.py", seed, DEVICE_VIEW_SWEEP_N)
    assert "failures 0" in out, out[-3000:]
