"""Arrays whose stage-1 code stream is prescribed symbol by symbol — TEST INFRASTRUCTURE (no tests, no fixtures).

Stage 1's Lorenzo code is the first difference of the lattice index, so x = 2 eb * prefix_sum(d) with eb a power of two codes to
exactly d + radius, in exactly the order chosen: the test prescribes the histogram AND the places of the rare symbols, which no
field does. The families below are the inputs on which Huffman constructions classically break: trees deeper than the length limit
(Fibonacci counts), massive ties (equal counts, powers of two), alphabets at the code-book paths' boundaries, and runs of a
thousand longest code words (a chunk near SZH_CHUNK_SYMS * limit bits). tests/test_crafted_codes_cpu.py holds every family to its
stated regime with the numpy model alone; tests/test_gpu_crafted_codes.py shows the streams to the kernels. The wide code books'
families (300 .. 65 535 symbols, the "balanced" order, sparse alphabets) are WIDE_FAMILIES below: tests/test_widebook_model_cpu.py,
tests/test_gpu_wide_books.py."""
import functools
import numpy as np

RADIUS = 32768
EB = 2.0 ** -10          # a power of two: q * 2 eb is exact in f32 and f64, and x / (2 eb) gives q back exactly
ORDERS = ("clustered", "shuffled", "periodic")   # (the orders of the families up to 2049 symbols; the wide families below: "balanced")
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

# ---- the wide code books (tests/widebook_model.py, tests/test_gpu_wide_books.py): alphabets of 300 .. 65 535 symbols in the "balanced" order.
# family -> (counts, the regime it binds); WIDE_REGIME: what tests/test_widebook_model_cpu.py holds each to without a GPU:
#   path        widebook_model.path
#   limit       the length limit of the book
#   tier        None: one class; else (keep, k) of the tier taken
#   and n_rare, rare_bits, floor (the class's weight is the floor's), binds (the unlimited tree is deeper than the limit), in_lds (the keys
#   of the construction fit the LDS queues and depth arrays: mk <= 16384)
SPACING = {}   # family -> the spacing of its symbols (default 1: dense)
WIDE_FAMILIES = {}
WIDE_REGIME = {}


def _wide(name, counts, text, spacing=1, **regime):
    WIDE_FAMILIES[name] = FAMILIES[name] = (list(counts), text)
    WIDE_REGIME[name] = regime
    if spacing != 1:
        SPACING[name] = spacing


def _geometric(m, hi, lo):
    """m counts falling from hi to lo in equal ratios"""
    return [int(round(hi * (float(lo) / hi) ** (i / float(m - 1)))) for i in range(m)]


_TAIL = [1] * 2500 + [2] * 1597          # 4097 rare symbols of 5694 occurrences; the tier rule's estimate of them: 2500 * 3 // 2 + 1597 * 3 = 8541
_TAIL_MASS = 2500 * 3 // 2 + 1597 * 3
_HEAD = _geometric(3000, 2040, 45)
for _m, _t in ((640, "the last alphabet of the small book by count"), (641, "the first of the wide book by count"),
               (4096, "CB_CLASS_MIN: the two-class form not considered"), (4097, "considered, both tiers rejected: the one-class form entered from the two-class one"),
               (15360, "tier 2 skipped: nothing to gain"), (15361, "tier 2 weighed and rejected"),
               (16384, "the last alphabet whose queues and depth arrays fit LDS"), (16385, "queues and depth arrays in global memory"),
               (65535, "the whole alphabet")):
    _wide("flat%d" % _m, [3] * _m, _t, path="small" if _m <= 640 else "wide1" if _m <= 4096 else "wide2", limit=24, tier=None, binds=False, in_lds=_m <= 16384)
FLAT_WIDE_CLUSTERED = ("flat640", "flat641", "flat4096", "flat4097", "flat15360", "flat15361", "flat16384", "flat16385")
_wide("sparse300", [3] * 300, "the wide book by span, 16-bit limit", spacing=16, path="wide1", limit=16, tier=None, binds=False, in_lds=True)
_wide("sparse600", [3] * 600, "the wide book by span", spacing=16, path="wide1", limit=24, tier=None, binds=False, in_lds=True)
_wide("sparse-fib16", [3] * 290 + [1200 * f for f in _fib(12)], "the wide book by span, the 16-bit limit binds", spacing=16,
      path="wide1", limit=16, tier=None, binds=True, in_lds=True)
_wide("tier1", _HEAD + _TAIL, "tier 1, 4097 rare symbols: 13 index bits, the class's weight is the floor's",
      path="wide2", limit=24, tier=(3072, 1), n_rare=4097, rare_bits=13, floor=True, binds=False, in_lds=True)
_wide("tier1-pow2", _HEAD + _TAIL[1:], "tier 1, 4096 rare symbols: 12 index bits, Kraft sum exactly 1, the class's weight its own",
      path="wide2", limit=24, tier=(3072, 1), n_rare=4096, rare_bits=12, floor=False, binds=False, in_lds=True)
_wide("tier1-keep", _geometric(3072, 2040, 45) + _TAIL, "3072 frequent symbols: above + oct[k] == keep",
      path="wide2", limit=24, tier=(3072, 1), n_rare=4097, rare_bits=13, floor=True, binds=False, in_lds=True)
_wide("tier1-keep+1", _geometric(3073, 2040, 45) + _TAIL, "3073 symbols above the tail: the walk stops four octaves higher, in the head",
      path="wide2", limit=24, tier=(3072, 5), n_rare=4375, rare_bits=13, floor=False, binds=False, in_lds=True)
_wide("tier1-heavy", _HEAD + [3] * 4097, "the rare class holds between 1/256 and 1/64 of the stream: its weight is its own",
      path="wide2", limit=24, tier=(3072, 1), n_rare=4097, rare_bits=13, floor=False, binds=False, in_lds=True)
# the licence at equality: the estimate 8541 * 64 == total, the head's first count taking up the difference; and one occurrence short of it
_EDGE = _geometric(3000, 300, 45)
_EDGE[0] += 64 * _TAIL_MASS - sum(_EDGE) - sum(_TAIL)
_wide("tier1-edge", _EDGE + _TAIL, "mass * 64 == total: tier 1 taken", path="wide2", limit=24, tier=(3072, 1), n_rare=4097, rare_bits=13, floor=False,
      binds=False, in_lds=True)
_wide("tier1-edge-1", [_EDGE[0] - 1] + _EDGE[1:] + _TAIL, "mass * 64 == total + 1: tier 1 rejected, tier 2 skipped", path="wide2", limit=24, tier=None,
      binds=False, in_lds=True)
_wide("tier2", [100000] + [64] * 12000 + [1] * 8000, "tier 1 rejected, tier 2 taken: 12 002 keys", path="wide2", limit=24, tier=(12288, 0), n_rare=8000,
      rare_bits=13, floor=False, binds=False, in_lds=True)
_wide("deep24w", [1] * 1100 + _fib(31)[15:], "1116 dense symbols, unlimited height 27 > 24: the wide path's clamp and repair three levels deep",
      path="wide1", limit=24, tier=None, binds=True, in_lds=True)
# tier 1's 4097 rare symbols under a Fibonacci head: the class — its weight is the floor's, 1/256 of the stream + 1 — takes the place of the
# term 17711, so the tree over the frequent symbols and the class is the chain itself: height 27
_wide("deep24w2", [f for f in _fib(31)[2:] if f != 17711] + [1] * 4097, "tier 1 AND the limit binds in the frequent class (height 27)", path="wide2",
      limit=24, tier=(3072, 0), n_rare=4097, rare_bits=13, floor=True, binds=True, in_lds=True)
# (deep30w — deep24w with a natural height of 30 — would have 15 M elements, beyond the 8 M a test's array may have: left out)
WIDE_1D = sorted(WIDE_FAMILIES)
# the 3-D form (f64, balanced): the N-d prefix sum of deltas within +-3549 stays below the lattice's 2^22
WIDE_SHAPE_ND = {"tier1": (33, 128, 384)}


def deltas_by_count(counts):
    """-> (delta per entry of `counts`): 0, +1, -1, +2, ... by falling count (ties: by position), so the running sum stays small"""
    counts = np.asarray(counts, dtype=np.int64)
    rank = np.empty(len(counts), dtype=np.int64)
    rank[np.argsort(-counts, kind="stable")] = np.arange(len(counts))
    return np.where(rank % 2 == 1, (rank + 1) // 2, -(rank // 2))


def balanced(deltas, rng):
    """-> the deltas in an order whose running sum stays within max(|sum of all deltas|, the largest |delta|): the next one comes from
    the shuffled negative pool while the running sum is positive, else from the positive pool (when one pool is empty the sum walks
    straight to its end value); the zeros, which move nothing, are dealt among the others at random"""
    deltas = np.asarray(deltas, dtype=np.int64)
    neg = rng.permutation(deltas[deltas < 0]).tolist()
    pos = rng.permutation(deltas[deltas > 0]).tolist()
    walk, run, i, j = [0] * (len(neg) + len(pos)), 0, 0, 0
    for t in range(len(walk)):
        if (run > 0 and i < len(neg)) or j == len(pos):
            v = neg[i]
            i += 1
        else:
            v = pos[j]
            j += 1
        run += v
        walk[t] = v
    out = np.zeros(deltas.size, dtype=np.int64)
    moved = np.ones(deltas.size, dtype=bool)
    moved[rng.choice(deltas.size, size=deltas.size - len(walk), replace=False)] = False
    out[moved] = walk
    return out


def delta_stream(counts, order, seed=1, spacing=1):
    """-> int64 deltas, sum(counts) of them, every entry i of `counts` counts[i] times, placed by `order`:
    clustered  rarest symbols first, every symbol's occurrences together: one run of the longest code words from element 0 on
    shuffled   a seeded shuffle
    periodic   the rarest occurrences at every 512-th position and its two neighbours, the others shuffled around them
    balanced   a seeded order whose running sum stays small (balanced()): alphabets of up to 65 535 symbols
    spacing: the deltas are multiples of it — a sparse alphabet, one symbol every `spacing` bins"""
    counts = np.asarray(counts, dtype=np.int64)
    delta = deltas_by_count(counts) * int(spacing)
    by_rarity = np.argsort(counts, kind="stable")
    stream = np.repeat(delta[by_rarity], counts[by_rarity])  # clustered
    n = stream.size
    rng = np.random.default_rng(seed)
    if order == "clustered":
        return stream
    if order == "shuffled":
        return rng.permutation(stream)
    if order == "balanced":
        return balanced(stream, rng)
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


@functools.lru_cache(maxsize=2)
def _deltas(family, order, counts):
    """(f32 and f64 of one family share the stream)"""
    return delta_stream(counts, order, spacing=SPACING.get(family, 1))


@functools.lru_cache(maxsize=4)
def _crafted(family, order, dtype_name, shape):
    counts = list(FAMILIES[family][0])
    if shape is not None:
        counts[int(np.argmax(counts))] += int(np.prod(shape)) - sum(counts)
    x, codes = array_from_deltas(_deltas(family, order, tuple(counts)), np.dtype(dtype_name), shape)
    x.setflags(write=False)
    codes.setflags(write=False)
    return x, codes


def crafted(family, order, dtype, shape=None):
    """-> (array, expected codes) of a family; cached, read-only"""
    return _crafted(family, order, np.dtype(dtype).name, None if shape is None else tuple(shape))


def histogram(family):
    """-> (counts by symbol over [sym_min, sym_max], sym_min) of a family's stream"""
    counts = np.asarray(FAMILIES[family][0], dtype=np.int64)
    sym = deltas_by_count(counts) * SPACING.get(family, 1) + RADIUS
    freq = np.zeros(int(sym.max() - sym.min()) + 1, dtype=np.int64)
    freq[sym - sym.min()] = counts
    return freq, int(sym.min())
