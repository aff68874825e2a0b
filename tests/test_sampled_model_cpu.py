"""tests/sampled_model.py without a device: the numpy rules for what the sampled-book path decides, held to a second, slower, plainly written form
on small arrays — loops over units and elements, a heap Huffman — and shown to catch three plain mistakes, each made once on a copy of the
model's input side (never in the kernels): stage 1 coding one plane too few in its last task, a sample unit placed one segment on, an unmet
value given its class's code word without the index bits."""
import heapq

import numpy as np
import pytest

import payload_checks
import sampled_model as SM
import szh_ref

EB = 1e-3


def _field(shape, seed=3, sigma=2e-3):
    """a smooth wave + noise: some thirty byte values, the rare ones met once or twice by a sample"""
    ax = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    f = sum(np.sin(2 * np.pi * g / (700.0 + 131 * i)) for i, g in enumerate(ax))
    f += np.random.default_rng(seed).normal(0.0, sigma, size=shape)
    return f.astype(np.float32)


# the smallest arrays a sample can be taken of have 1024 segments; these have 2 .. 3 per unit, so the hash inside a unit's stride matters.
# 3-D with y % 4 = 3 and z % 16 = 1; 2-D with rows % 4 = 1; 1-D
SHAPES = [(17, 43, 3 * 256), (2053, 256), (2051 * 256,)]


@pytest.fixture(scope="module", params=SHAPES, ids=["3d", "2d", "1d"])
def coded(request):
    shape = request.param
    a = _field(shape)
    a.reshape(-1)[5000] += 0.7  # far deltas: byte 255
    q, d, codes, bad, far = szh_ref.dualquant(a, EB, narrow=True)
    return dict(shape=shape, a=a, q=q, d=d, codes=codes, far=far)


def slow_counts(q, shape):
    """unit by unit, element by element: the Lorenzo stencil over the lattice values with zeros outside the array, the byte, its count"""
    d3 = (1,) * (3 - len(shape)) + tuple(shape)
    q3 = q.reshape(d3)
    nz, ny, nx = d3
    nseg = nz * ny * nx // 256
    stride = nseg // 1024
    counts = [0] * 256
    at = lambda z, y, x: int(q3[z, y, x]) if z >= 0 and y >= 0 and x >= 0 else 0  # noqa: E731
    for u in range(1024):
        seg = u * nseg // 1024 + (((u * 2654435761) % (1 << 32)) >> 8) % stride
        per_row = nx // 256
        row, x0 = seg // per_row, (seg % per_row) * 256
        z, y = row // ny, row % ny
        for x in range(x0, x0 + 256):
            delta = (at(z, y, x) - at(z, y, x - 1) - at(z, y - 1, x) + at(z, y - 1, x - 1)
                     - at(z - 1, y, x) + at(z - 1, y, x - 1) + at(z - 1, y - 1, x) - at(z - 1, y - 1, x - 1))
            t = delta + 127
            counts[t if 0 <= t <= 254 else 255] += 1
    return np.array(counts, dtype=np.int64)


def slow_book(counts, index_bits=True):
    """-> 256 code lengths: a heap Huffman over 4 * count per met value and one class of weight n_un for the unmet ones, whose code words are
    the class's followed by ceil(log2(n_un)) index bits. (No length limit: for books whose tree is at most 16 deep.)"""
    met = [t for t in range(256) if counts[t]]
    n_un = 256 - len(met)
    nodes = [(4 * int(counts[t]), i, [t]) for i, t in enumerate(met)]
    if n_un:
        nodes.append((n_un, len(nodes), ["class"]))
    depth = {leaf: 0 for _, _, leaves in nodes for leaf in leaves}
    heapq.heapify(nodes)
    tick = len(nodes)
    while len(nodes) > 1:
        w1, _, l1 = heapq.heappop(nodes)
        w2, _, l2 = heapq.heappop(nodes)
        for leaf in l1 + l2:
            depth[leaf] += 1
        heapq.heappush(nodes, (w1 + w2, tick, l1 + l2))
        tick += 1
    bits = 0
    while (1 << bits) < n_un:
        bits += 1
    lens = np.zeros(256, dtype=np.int64)
    for t in range(256):
        lens[t] = depth[t] if counts[t] else depth["class"] + (bits if index_bits else 0)
    return lens


def limited_book(counts):
    """-> 256 code lengths of the 16-bit optimum over met values and class (package-merge; where the tree is at most 16 deep, a Huffman code's cost)"""
    w, met, n_un = SM.class_weights(counts)
    pm = szh_ref.package_merge_lengths(w, 16)
    lens = np.zeros(256, dtype=np.int64)
    lens[met] = pm[:len(pm) - (1 if n_un else 0)]
    if n_un:
        lens[~met] = pm[-1] + SM.index_bits(n_un)
    return lens


def test_the_probe_rule(coded):
    d = coded["d"].reshape(-1)
    big = n_samples = 0
    for i in range(d.size):
        if i % 32768 < 64:
            n_samples += 1
            big += abs(int(d[i])) > 127
    assert SM.probe(coded["d"]) == (big, n_samples, big * 4096 <= n_samples)
    assert SM.narrow_codes(coded["d"], 32768) == (big * 4096 <= n_samples) and not SM.narrow_codes(coded["d"], 64)


def test_the_probe_counts_a_far_delta_in_its_window_and_none_outside():
    d = np.zeros(3 * 32768 + 10, dtype=np.int32)
    d[32768 + 64] = 500   # the first element behind a window
    d[2 * 32768 - 1] = -500
    assert SM.probe(d) == (0, 3 * 64 + 10, True)
    d[32768 + 63] = 128
    d[3 * 32768 + 9] = -128
    assert SM.probe(d) == (2, 3 * 64 + 10, False)  # 2 * 4096 > 202


def probed_stencils(shape):
    """element by element: the flat indices of every value in the Lorenzo stencil of a probed element (neighbours outside the array: none)"""
    import itertools
    n = int(np.prod(shape))
    seen = set()
    for i in range(n):
        if i % 32768 >= 64:
            continue
        at = np.unravel_index(i, shape)
        for step in itertools.product((0, 1), repeat=len(shape)):
            c = [int(v) - s for v, s in zip(at, step)]
            if min(c) >= 0:
                seen.add(int(np.ravel_multi_index(c, shape)))
    return seen


def test_the_16_bit_licence_is_about_the_probed_stencils(coded):
    q, a, shape = coded["q"], coded["a"], coded["shape"]
    assert SM.q16_licensed(q, a, EB) and not SM.q16_voids(a, EB)
    seen = probed_stencils(shape)
    inside = min(i for i in seen if i > 40000)   # the far corner of a later window's stencils
    outside = inside - 1
    assert outside not in seen
    for value, voids in ((2048 * 2 * EB, False), (4096 * 2 * EB, True), (np.nan, True), (np.inf, True), (1e30, True)):
        b = a.copy()
        b.reshape(-1)[inside] = value
        qb = szh_ref.dualquant(b, EB, narrow=True)[0]
        assert not SM.q16_licensed(qb, b, EB), value
        assert SM.q16_voids(b, EB) == voids, value
        c = a.copy()
        c.reshape(-1)[outside] = value
        assert SM.q16_licensed(szh_ref.dualquant(c, EB, narrow=True)[0], c, EB), value
        assert SM.q16_voids(c, EB) == voids, value


def test_the_dispatchers_rule():
    f32, f64 = np.float32, np.float64
    assert SM.takes_sampled_book((1 << 22,), f32, 128) and SM.takes_sampled_book((2, 1 << 21), f64, 32768) and SM.takes_sampled_book((16, 1024, 256), f32, 512)
    assert not SM.takes_sampled_book(((1 << 22) - 256,), f32, 32768)   # one segment short
    assert not SM.takes_sampled_book((64, 256, 260), f32, 32768)       # rows of no whole segments
    assert not SM.takes_sampled_book((2, 32, 256, 256), f32, 32768)    # rank 4
    assert not SM.takes_sampled_book((64, 256, 256), f32, 64)          # quantbinCnt 128


def test_the_sample_against_the_loop(coded):
    assert np.array_equal(SM.sample_counts(coded["d"], coded["shape"]), slow_counts(coded["q"], coded["shape"]))


def test_check_book_takes_the_heap_huffman_and_refuses_other_books(coded):
    counts = SM.sample_counts(coded["d"], coded["shape"])
    lens = slow_book(counts)
    fig = SM.check_book(lens, counts)
    assert fig["height"] <= 16 and not fig["limit_binds"] and fig["cost"] == fig["huffman_cost"] and fig["excess"] == 0.0
    met = np.nonzero(counts)[0]
    a, b = met[np.argmax(counts[met])], met[np.argmin(counts[met])]
    swapped = lens.copy()
    swapped[a], swapped[b] = lens[b], lens[a]   # a valid prefix code that costs more
    assert lens[a] != lens[b]
    with pytest.raises(AssertionError, match="Huffman"):
        SM.check_book(swapped, counts)
    shorter = lens.copy()
    shorter[a] -= 1
    with pytest.raises(AssertionError, match="Kraft"):
        SM.check_book(shorter, counts)


def test_check_book_where_the_limit_binds():
    """Fibonacci counts: a tree 21 deep. A book of the 16-bit optimum passes with excess 0, one that lengthens a frequent value has a positive
    excess, one cheaper than the optimum is no code of that limit"""
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    counts = np.zeros(256, dtype=np.int64)
    counts[100:124] = fib
    counts[127] = 262144 - counts.sum()
    w, met, n_un = SM.class_weights(counts)
    assert szh_ref.huffman_cost(w)[1] > 16
    pm = szh_ref.package_merge_lengths(w, 16)
    lens = np.zeros(256, dtype=np.int64)
    lens[met] = pm[:-1]
    lens[~met] = pm[-1] + SM.index_bits(n_un)
    fig = SM.check_book(lens, counts)
    assert fig["limit_binds"] and fig["excess"] == 0.0 and fig["cost"] == fig["pm_cost"] > fig["huffman_cost"]
    worse = lens.copy()
    worse[127] += 1
    assert SM.check_book(worse, counts)["excess"] > 0.0
    unlimited = np.zeros(256, dtype=np.int64)
    unlimited[:] = slow_book(counts)
    with pytest.raises(AssertionError):
        SM.check_book(unlimited, counts)  # (words of more than 16 bits for values the sample met)


# ---- three plain mistakes, each on a copy of the model's input side ------------------------------------------------------------------------
def test_mistake_one_plane_too_few_in_the_last_task(coded):
    """stage 1 deals 16 planes a task; a last task that codes z % 16 - 1 planes leaves the array's last plane (1-D, 2-D: its last row of tasks —
    the last 256 elements) as the code array held them: the code comparison names the place"""
    shape, codes = coded["shape"], coded["codes"]
    device = codes.copy()
    if len(shape) == 3:
        device[-1] = 0
    else:
        device.reshape(-1)[-256:] = 0
    payload_checks.same_codes(codes, codes.copy(), shape)
    with pytest.raises(AssertionError, match="quantisation codes differ"):
        payload_checks.same_codes(device, codes, shape)


def test_mistake_a_sample_unit_one_segment_on(coded):
    """a device whose units sit one segment on builds a valid book of another sample: check_book refuses it against the model's counts"""
    counts = SM.sample_counts(coded["d"], coded["shape"])
    moved = SM.sample_counts(coded["d"], coded["shape"], shift=1)
    assert not np.array_equal(counts, moved)
    lens = limited_book(moved)
    SM.check_book(lens, moved)
    with pytest.raises(AssertionError):
        SM.check_book(lens, counts)


def test_mistake_an_unmet_value_without_its_index_bits(coded):
    counts = SM.sample_counts(coded["d"], coded["shape"])
    assert 2 <= 256 - np.count_nonzero(counts)
    with pytest.raises(AssertionError):
        SM.check_book(slow_book(counts, index_bits=False), counts)
