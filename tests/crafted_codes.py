"""Arrays whose stage-1 code stream is prescribed symbol by symbol — TEST INFRASTRUCTURE (no tests, no fixtures).

Stage 1's Lorenzo code is the first difference of the lattice index, so x = 2 eb * prefix_sum(d) with eb a power of two codes to
exactly d + radius, in exactly the order chosen: the test prescribes the histogram AND the places of the rare symbols, which no
field does. The families below are the inputs on which Huffman constructions classically break: trees deeper than the length limit
(Fibonacci counts), massive ties (equal counts, powers of two), alphabets at the code-book paths' boundaries, and runs of a
thousand longest code words (a chunk near SZH_CHUNK_SYMS * limit bits). tests/test_crafted_codes_cpu.py holds every family to its
stated regime with the numpy model alone; tests/test_gpu_crafted_codes.py shows the streams to the kernels."""
import functools
import numpy as np

RADIUS = 32768
EB = 2.0 ** -10          # a power of two: q * 2 eb is exact in f32 and f64, and x / (2 eb) gives q back exactly
ORDERS = ("clustered", "shuffled", "periodic")
PERIOD = 512             # = szh_ref.UNIT: the periodic order's rare symbols sit on the unit and chunk borders


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


# family -> (counts, what it binds)
FAMILIES = {
    # (a small alphabet's book has margins, szh_ref.book_symbols: sixteen more symbols counted once each. Under Fibonacci counts from 1
    # they flatten the tree below the limit; from 13 on they hang below the chain as one subtree of height 4)
    "fib17": (_fib(23)[6:], "13, 21 ... 28657: unlimited height 21 > 16 with the book's margins; small path, narrow codes"),
    "pow2": ([1] + [1 << k for k in range(18)], "height 18 > 16; all ties"),
    "deep16": ([3] * 400 + [1200 * f for f in _fib(12)], "412 symbols; clustered, a chunk reaches >= 90 % of 1024 * 16 bits"),
    # ... the same with 516 fewer of the most frequent symbol: the last chunk holds 300 symbols, fewer than a unit
    "deep16-ragged": ([3] * 400 + [1200 * f for f in _fib(11)] + [1200 * 144 - 516], "deep16 with a last chunk shorter than a unit"),
    # one more Fibonacci term: every optimal code is exactly 16 bits deep — the limit neither binds nor leaves a bit to spare
    "edge16": ([3] * 400 + [1200 * f for f in _fib(13)], "413 symbols; the optimal code needs all 16 bits and no more"),
    "deep24": ([1] * 500 + [512 * f for f in _fib(18)], "518 symbols; unlimited height 27 > 24"),
    "two": ([1, 4999], "one-bit codes; margins of the small book"),
    "dominant": ([200000] + [1] * 300, "one-bit head, deep flat tail"),
}
FLAT_SIZES = (255, 256, 257, 511, 512, 513, 2047, 2048, 2049)
for _m in FLAT_SIZES:
    FAMILIES["flat%d" % _m] = ([3] * _m, "path boundary; all ties; fewer than two chunks")

FAMILIES_1D = sorted(FAMILIES)
# the array of the sampled book (2^22 elements or more, rows of whole 256-element segments, one-byte codes): fib17's counts 56 times, 2-D f32
SAMPLED_FAMILY, SAMPLED_SHAPE = "fib17x56", (2051, 2048)
FAMILIES[SAMPLED_FAMILY] = ([56 * c for c in FAMILIES["fib17"][0]], "fib17 at the sampled book's size: a book that never saw the rare run")

# the 3-D forms (f64, shuffled): x is the N-d prefix sum of d — the tiled / marching stage-1 kernels and the strided scans
# (a shape with more elements than the family: the most frequent symbol that many more times)
SHAPES_3D = {"fib17": (19, 30, 132), "deep16": (29, 60, 260)}


def deltas_by_count(counts):
    """-> (delta per entry of `counts`): 0, +1, -1, +2, ... by falling count (ties: by position), so the running sum stays small"""
    counts = np.asarray(counts, dtype=np.int64)
    rank = np.empty(len(counts), dtype=np.int64)
    rank[np.argsort(-counts, kind="stable")] = np.arange(len(counts))
    return np.where(rank % 2 == 1, (rank + 1) // 2, -(rank // 2))


def delta_stream(counts, order, seed=1):
    """-> int64 deltas, sum(counts) of them, every entry i of `counts` counts[i] times, placed by `order`:
    clustered  rarest symbols first, every symbol's occurrences together: one run of the longest code words from element 0 on
    shuffled   a seeded shuffle
    periodic   the rarest occurrences at every 512-th position and its two neighbours, the others shuffled around them"""
    counts = np.asarray(counts, dtype=np.int64)
    delta = deltas_by_count(counts)
    by_rarity = np.argsort(counts, kind="stable")
    stream = np.repeat(delta[by_rarity], counts[by_rarity])  # clustered
    n = stream.size
    rng = np.random.default_rng(seed)
    if order == "clustered":
        return stream
    if order == "shuffled":
        return rng.permutation(stream)
    if order == "periodic":
        k = np.arange(PERIOD, n - 1, PERIOD)
        places = np.stack([k - 1, k, k + 1], axis=1).reshape(-1)
        out = np.empty(n, dtype=np.int64)
        rest = np.ones(n, dtype=bool)
        rest[places] = False
        out[places] = rng.permutation(stream[:places.size])
        out[rest] = rng.permutation(stream[places.size:])
        return out
    raise ValueError(order)


def array_from_deltas(d, dtype, shape=None):
    """-> (array of `shape` (default 1-D) whose Lorenzo deltas are d in raster order, expected codes uint16 flat)"""
    d = np.asarray(d, dtype=np.int64)
    shape = (d.size,) if shape is None else tuple(shape)
    q = d.reshape(shape)
    for ax in range(len(shape)):
        q = np.cumsum(q, axis=ax)
    assert int(np.abs(q).max()) < 1 << 22 and int(np.abs(d).max()) < RADIUS
    x = (q.astype(np.float64) * (2.0 * EB)).astype(dtype)
    return x, (d + RADIUS).astype(np.uint16)


def assert_prescribed(x, codes):
    """precondition (a): the model of stage 1 (szh_ref.dualquant) codes x to exactly `codes`, with no value outlier and no listed delta
    — in the one-byte form too where every delta fits it"""
    import szh_ref
    for narrow in (False, True):
        if narrow and int(np.abs(codes.astype(np.int64) - RADIUS).max()) > 127:
            continue
        _, _, got, bad, far = szh_ref.dualquant(x, EB, narrow=narrow)
        assert np.array_equal(got.reshape(-1), codes), "the array does not code to the prescribed stream"
        assert not bad.any() and not far.any()


@functools.lru_cache(maxsize=4)
def _crafted(family, order, dtype_name, shape):
    counts = list(FAMILIES[family][0])
    if shape is not None:
        counts[int(np.argmax(counts))] += int(np.prod(shape)) - sum(counts)
    x, codes = array_from_deltas(delta_stream(counts, order), np.dtype(dtype_name), shape)
    x.setflags(write=False)
    codes.setflags(write=False)
    return x, codes


def crafted(family, order, dtype, shape=None):
    """-> (array, expected codes) of a family; cached, read-only"""
    return _crafted(family, order, np.dtype(dtype).name, None if shape is None else tuple(shape))


def histogram(family):
    """-> (counts by symbol over [sym_min, sym_max], sym_min) of a family's stream"""
    counts = np.asarray(FAMILIES[family][0], dtype=np.int64)
    sym = deltas_by_count(counts) + RADIUS
    freq = np.zeros(int(sym.max() - sym.min()) + 1, dtype=np.int64)
    freq[sym - sym.min()] = counts
    return freq, int(sym.min())
