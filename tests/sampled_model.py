"""numpy rules for what the device decides on the sampled-book Lorenzo path — TEST INFRASTRUCTURE (no tests, no fixtures).

Everything here runs on the CPU and is built on szh_ref.dualquant's lattice values `q` and Lorenzo deltas `d`:
  probe(d)                 the probe's count of far deltas and the one-byte rule                  (k_probe, szk_is_narrow)
  narrow_codes(d, radius)  ... with the radius rule of the dispatcher in front                     (lorenzo_k1: mode.allow)
  q16_licensed(q, a, eb)   the probed stencil values lie within +-2047 lattice steps, all finite  (probe counter [3])
  q16_voids(a, eb)         a value the 16-bit form of stage 1 does not take: the call is repeated (Q16_LIM, q16_flag)
  takes_sampled_book(...)  the dispatcher's rule for the sampled book                              (lorenzo_k1)
  sample_segments(shape)   the 1024 segments of the sample, a function of the extents alone        (samp_unit_place)
  sample_counts(d, shape)  the 256 counts of the sample                                            (samp_take)
  check_book(lens, counts) the payload's lengths table against those counts                        (samp_book)
tests/test_sampled_model_cpu.py holds these rules to a second, plainly written form."""
import numpy as np

import szh_ref

PROBE_STRIDE, PROBE_RUN = 32768, 64   # the probe looks at 64 consecutive elements of every 32768
SAMP_UNITS, SEG = 1024, 256           # sample units of one array; a unit is one 256-element row segment
SAMP_MIN_ELEMS = 1 << 22
SEEN_LEN = 16                         # longest code word of a byte value the sample met
Q16_LIM, Q16_PROBE_LIM = 4095.0, 2047.0
HASH = 2654435761


def probe_positions(n):
    """-> the flat indices the probe reads"""
    i = (np.arange(0, n, PROBE_STRIDE, dtype=np.int64)[:, None] + np.arange(PROBE_RUN, dtype=np.int64)[None, :]).reshape(-1)
    return i[i < n]


def probe(d):
    """-> (big, n_samples, one_byte): the probe's count of |delta| > 127 over the first 64 elements of every 32768, the number of probed
    elements, and the rule big * 4096 <= n_samples"""
    flat = np.asarray(d).reshape(-1)
    n = flat.size
    pos = probe_positions(n)
    n_samples = (n // PROBE_STRIDE) * PROBE_RUN + min(PROBE_RUN, n % PROBE_STRIDE)
    assert n_samples == pos.size
    big = int(np.count_nonzero(np.abs(flat[pos].astype(np.int64)) > 127))
    return big, n_samples, big * 4096 <= n_samples


def narrow_codes(d, radius):
    """one-byte codes: a radius of at least 128 and the probe's rule"""
    return radius >= 128 and probe(d)[2]


def _scaled(a, eb):
    """fl(a * fl(1 / 2eb)) in the array's type, as stage 1 computes it"""
    a = np.ascontiguousarray(a)
    recip = np.float32(1.0 / (2.0 * eb)) if a.dtype == np.float32 else 1.0 / (2.0 * eb)
    with np.errstate(invalid="ignore", over="ignore"):
        return (a * recip).astype(a.dtype)


def q16_licensed(q, a=None, eb=None):
    """the licence of stage 1's 16-bit form (f32 streams): every value in the Lorenzo stencil of a probed element lies within +-2047 lattice
    steps. With the array given, the rule is the probe's own: the scaled value a / 2eb itself within +-2047 and finite (a NaN has q = 0)."""
    q = np.asarray(q)
    m = np.zeros(q.size, dtype=bool)
    m[probe_positions(q.size)] = True
    m = m.reshape(q.shape)
    for ax in range(q.ndim):  # the stencil's corners: one step down along every subset of the axes
        lo = [slice(None)] * q.ndim
        hi = [slice(None)] * q.ndim
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        m[tuple(lo)] |= m[tuple(hi)]
    ok = bool(np.all(np.abs(q[m].astype(np.int64)) <= int(Q16_PROBE_LIM)))
    if a is not None:
        s = _scaled(a, eb)[m]
        with np.errstate(invalid="ignore"):
            ok = ok and bool(np.all(np.abs(s) <= Q16_PROBE_LIM))
    return ok


def q16_voids(a, eb):
    """the 16-bit form voids its launch (and the call is repeated in the one-byte form) on a value that is not finite or whose lattice
    value rint(a / 2eb) lies beyond +-4095"""
    assert a.dtype == np.float32
    s = _scaled(a, eb)
    magic = np.float32(12582912.0)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (s + magic).astype(np.float32) - magic
        return bool(np.any(~(np.abs(r) <= np.float32(Q16_LIM))))


def takes_sampled_book(shape, dtype, radius, n=None):
    """the dispatcher's rule: rank <= 3, rows of whole 256-element segments, at least 2^22 elements, a radius of at least 128 (the stream
    must also turn out to have one-byte codes: narrow_codes). dtype: f32 and f64 both take it."""
    n = int(np.prod(shape)) if n is None else int(n)
    assert np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.float64))
    return len(shape) <= 3 and shape[-1] % SEG == 0 and n >= SAMP_MIN_ELEMS and radius >= 128


def sample_segments(shape, shift=0):
    """-> the segment (index into the array cut into 256-element pieces, raster order) of each of the 1024 units:
    u * nseg // 1024 + ((u * 2654435761 mod 2^32) >> 8) % (nseg // 1024). shift: added to every segment (tests of the tests)"""
    n = int(np.prod(shape))
    assert shape[-1] % SEG == 0
    nseg = n // SEG
    stride = nseg // SAMP_UNITS
    assert stride >= 1
    u = np.arange(SAMP_UNITS, dtype=np.uint64)
    h = ((u * np.uint64(HASH)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)
    seg = (u * np.uint64(nseg)) // np.uint64(SAMP_UNITS) + h % np.uint64(stride)
    return seg.astype(np.int64) + int(shift)


def sample_counts(d, shape, shift=0):
    """-> the 256 counts of the sample: every element of a unit gives the byte t = delta + 127 where that lies in 0 .. 254, else 255"""
    flat = np.asarray(d).reshape(-1).astype(np.int64)
    seg = sample_segments(shape, shift)
    idx = (seg[:, None] * SEG + np.arange(SEG, dtype=np.int64)[None, :]).reshape(-1)
    t = flat[idx] + 127
    t = np.where((t >= 0) & (t <= 254), t, 255)
    return np.bincount(t, minlength=256).astype(np.int64)


def class_weights(counts):
    """-> (weights of the Huffman code over the sample, met mask, n_un): 4 * count per byte value the sample met, then — where there are
    values it did not meet — one class of weight n_un that stands for all of them"""
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.shape == (256,) and counts.sum() == SAMP_UNITS * SEG
    met = counts > 0
    n_un = int(256 - met.sum())
    w = 4 * counts[met]
    if n_un:
        w = np.concatenate([w, [n_un]])
    return w, met, n_un


def index_bits(n_un):
    """ceil(log2(n_un)): the bits that tell an unmet value from the others of its class"""
    return 0 if n_un <= 1 else int(n_un - 1).bit_length()


def check_book(lens, counts):
    """the lengths table of a sampled-book payload (256 entries, byte value t = symbol sym_min + t) against the sample's counts.
    -> dict(height, limit_binds, cost, huffman_cost, pm_cost, excess): excess = bits per sampled symbol over the 16-bit optimum
    (package-merge) where the limit binds, else 0. Raises AssertionError on a book that breaks a rule."""
    lens = np.asarray(lens).astype(np.int64)
    assert lens.shape == (256,), "a sampled book has 256 lengths"
    w, met, n_un = class_weights(counts)
    assert np.all(lens[met] >= 1) and np.all(lens[met] <= SEEN_LEN), "a value the sample met has a code word of %d bits" % int(lens[met].max())
    lv = lens[met]
    if n_un:
        un = lens[~met]
        assert np.all(un == un[0]), "the unmet values' code words differ in length: %s" % sorted(set(un.tolist()))
        lc = int(un[0]) - index_bits(n_un)
        assert 1 <= lc <= SEEN_LEN, "an unmet value has %d bits: not the class's code word (1 .. 16 bits) + %d index bits" % (int(un[0]), index_bits(n_un))
        lv = np.concatenate([lv, [lc]])
    assert np.all(lens >= 1) and lens.max() <= szh_ref.MAX_LEN
    kraft_units = int(np.sum(np.int64(1) << (szh_ref.MAX_LEN - lens)))
    assert kraft_units <= 1 << szh_ref.MAX_LEN, "Kraft sum %d / 2^24 > 1" % kraft_units
    tree_units = int(np.sum(np.int64(1) << (SEEN_LEN - lv)))
    assert tree_units <= 1 << SEEN_LEN, "Kraft sum of the code over met values and class %d / 2^16 > 1" % tree_units
    cost = int((w * lv).sum())
    huff, height = szh_ref.huffman_cost(w)
    out = dict(height=height, limit_binds=height > SEEN_LEN, cost=cost, huffman_cost=huff, pm_cost=huff, excess=0.0)
    if height <= SEEN_LEN:
        assert cost == huff, "the book costs %d bits over the sample, the Huffman code %d" % (cost, huff)
    else:
        pm = szh_ref.package_merge_lengths(w, SEEN_LEN)
        out["pm_cost"] = int((w * pm).sum())
        assert cost >= out["pm_cost"], "the book costs less than the 16-bit optimum: not a code of that limit"
        out["excess"] = (cost - out["pm_cost"]) / float(w.sum())
    return out
