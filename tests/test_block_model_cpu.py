"""CPU tests (-m "not gpu") of the numpy model of the block decoder (tests/szh_ref.py) against its own definitions, so that the model
can run at the sizes of tests/test_gpu_blkdec_rounds.py: the whole-block inverse of a Lorenzo block (differences, the block's deltas,
cumulative sums in int64) against the element-by-element stencil, a run of regression blocks against a block at a time, the code
positions against the block walk, reconstruct_blocks against a walk over single blocks made of the definitions alone, and the
unit-parallel Huffman and side-section readers against the bit-by-bit ones. No library and no device needed."""
import itertools

import numpy as np
import pytest

import szh_ref

DELTA_MAX = 1 << 30


def _both_forms(rng, origin, extents, order):
    """a padded lattice array of random values around and behind the block (the halo the block reads, and cells it must not touch),
    deltas up to +-2^30 -> the array after the element-wise and after the whole-block form"""
    shape = tuple(o + e + 2 + pad for o, e, pad in zip(origin, extents, (1, 2, 3)))
    q = rng.integers(-DELTA_MAX, DELTA_MAX, size=shape, endpoint=True).astype(np.int64)
    delta = rng.integers(-DELTA_MAX, DELTA_MAX, size=extents, endpoint=True).astype(np.int64)
    qa, qb = q.copy(), q.copy()
    szh_ref.lorenzo_block_elementwise(qa, delta, origin, extents, order)
    szh_ref.lorenzo_block(qb, delta, origin, extents, order)
    inner = tuple(slice(o + 2, o + 2 + e) for o, e in zip(origin, extents))
    outside = np.ones(shape, dtype=bool)
    outside[inner] = False
    assert np.array_equal(qa[outside], q[outside]) and np.array_equal(qb[outside], q[outside]), "a form wrote outside its block"
    return qa, qb


@pytest.mark.parametrize("order", [1, 2])
def test_whole_block_form_equals_the_stencil_in_3d(order):
    """every extent 1 .. 8 per axis, random halos, origins off zero"""
    rng = np.random.default_rng(100 + order)
    for extents in itertools.product(range(1, 9), repeat=3):
        origin = tuple(int(v) for v in rng.integers(0, 3, size=3))
        qa, qb = _both_forms(rng, origin, extents, order)
        assert np.array_equal(qa, qb), (order, origin, extents)


@pytest.mark.parametrize("order", [1, 2])
def test_whole_block_form_equals_the_stencil_in_2d_and_1d(order):
    """as the model sees arrays of fewer dimensions: (1, ey, ex) and (1, 1, n), every extent 1 .. 17; with random halos, and with the
    zero halo layers such an array has along its missing axes"""
    rng = np.random.default_rng(200 + order)
    shapes = [(1, ey, ex) for ey in range(1, 18) for ex in range(1, 18)] + [(1, 1, n) for n in range(1, 18)]
    for extents in shapes:
        origin = (0, 0 if extents[1] == 1 else int(rng.integers(0, 3)), int(rng.integers(0, 4)))
        qa, qb = _both_forms(rng, origin, extents, order)
        assert np.array_equal(qa, qb), (order, origin, extents)
        # zero layers below z (and below y in 1-D), as in reconstruct_blocks' array
        shape = tuple(o + e + 2 for o, e in zip(origin, extents))
        q = rng.integers(-DELTA_MAX, DELTA_MAX, size=shape, endpoint=True).astype(np.int64)
        q[:2] = 0
        if extents[1] == 1:
            q[:, :2] = 0
        delta = rng.integers(-DELTA_MAX, DELTA_MAX, size=extents, endpoint=True).astype(np.int64)
        qa, qb = q.copy(), q.copy()
        szh_ref.lorenzo_block_elementwise(qa, delta, origin, extents, order)
        szh_ref.lorenzo_block(qb, delta, origin, extents, order)
        assert np.array_equal(qa, qb), (order, origin, extents)


def test_a_run_of_lorenzo_blocks_is_one_box():
    """blocks of one order side by side along x obey one recurrence: block by block and as one box give the same array"""
    rng = np.random.default_rng(3)
    for order, B, nblk, tail in ((1, 4, 5, 0), (2, 4, 3, 3), (1, 6, 2, 1), (2, 8, 4, 5)):
        ex = B * nblk + tail
        q = rng.integers(-1000, 1000, size=(2 + 3, 2 + B, 2 + 5 + ex), endpoint=True).astype(np.int64)
        delta = rng.integers(-DELTA_MAX, DELTA_MAX, size=(3, B, ex), endpoint=True).astype(np.int64)
        qa, qb = q.copy(), q.copy()
        for x0 in range(0, ex, B):
            e = min(B, ex - x0)
            szh_ref.lorenzo_block_elementwise(qa, delta[:, :, x0:x0 + e], (0, 0, 5 + x0), (3, B, e), order)
        szh_ref.lorenzo_block(qb, delta, (0, 0, 5), (3, B, ex), order)
        assert np.array_equal(qa, qb)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_run_of_regression_blocks_equals_block_by_block(T):
    rng = np.random.default_rng(4)
    radius = 32768
    for (ez, ey), B, nblk, tail, nd1, eb in (((6, 6), 6, 4, 0, 4, 1e-3), ((1, 4), 4, 7, 3, 3, 0.15), ((1, 1), 8, 9, 5, 2, 1e-4), ((5, 3), 6, 1, 2, 4, 2e-2)):
        ex = B * nblk + tail
        nb = nblk + (1 if tail else 0)
        cc = rng.integers(radius - 300, radius + 300, size=(ez, ey, ex)).astype(np.int64)
        cc[rng.random(cc.shape) < 0.05] = 0  # (code 0: unpredictable, the value comes from the list)
        lcs = rng.integers(-(1 << 20), 1 << 20, size=(nb, 4)).astype(np.int64)
        lcs[0, 3] = (1 << 40) if T == np.float64 else (1 << 26)  # (values beyond the lattice's range in f32)
        qt, val = szh_ref.regression_run(cc, lcs, B, eb, radius, T, nd1)
        assert val.dtype == T and qt.dtype == np.int64
        for b in range(nb):
            sl = slice(b * B, min((b + 1) * B, ex))
            q1, v1 = szh_ref.regression_block(cc[:, :, sl], lcs[b], B, eb, radius, T, nd1)
            assert np.array_equal(q1, qt[:, :, sl]) and np.array_equal(v1.view(np.uint8), val[:, :, sl].view(np.uint8)), (T, B, b)


@pytest.mark.parametrize("dims,B", [((7, 9, 11), 5), ((1, 1, 37), 8), ((1, 20, 33), 4), ((6, 6, 6), 6), ((13, 2, 5), 6)])
def test_code_positions_equal_the_block_walk(dims, B):
    want = np.zeros(dims, dtype=np.int64)
    pos = 0
    for z0, y0, x0 in itertools.product(range(0, dims[0], B), range(0, dims[1], B), range(0, dims[2], B)):
        e = [min(B, d - o) for d, o in zip(dims, (z0, y0, x0))]
        m = e[0] * e[1] * e[2]
        want[z0:z0 + e[0], y0:y0 + e[1], x0:x0 + e[2]] = np.arange(pos, pos + m).reshape(e)
        pos += m
    assert np.array_equal(szh_ref.block_positions(dims, B), want)


def _by_definition(h, sec, codes, sel, coef):
    """the block decoder a block at a time, from the definitions alone"""
    T = np.float32 if h["dtype"] == 0 else np.float64
    dz, dy, dx = h["dims"][1:]
    B, eb, radius = h["blk_edge"], h["eb"], h["radius"]
    dflat = np.where(codes == 0, 0, codes.astype(np.int64) - radius).astype(np.int64)
    dflat[sec["dout_idx"].astype(np.int64)] = sec["dout_val"]
    q = np.zeros((dz + 2, dy + 2, dx + 2), dtype=np.int64)
    out = np.zeros((dz, dy, dx), dtype=T)
    pos, r = 0, 0
    for bz, by, bx in itertools.product(*[range(n) for n in sel.shape]):
        o = (bz * B, by * B, bx * B)
        e = tuple(min(B, d - v) for d, v in zip((dz, dy, dx), o))
        m = e[0] * e[1] * e[2]
        blk = tuple(slice(v, v + n) for v, n in zip(o, e))
        pad = tuple(slice(v + 2, v + 2 + n) for v, n in zip(o, e))
        if sel[bz, by, bx] == 2:
            q[pad], out[blk] = szh_ref.regression_block(codes[pos:pos + m].reshape(e).astype(np.int64), coef[r], B, eb, radius, T, h["ndim"] + 1)
            r += 1
        else:
            szh_ref.lorenzo_block_elementwise(q, dflat[pos:pos + m].reshape(e), o, e, int(sel[bz, by, bx]) + 1)
            out[blk] = q[pad].astype(T) * T(2.0 * eb)
        pos += m
    x = out.reshape(-1)
    x[sec["vout_idx"].astype(np.int64)] = sec["vout_val"]
    return x


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("dims,B,ndim", [((13, 20, 27), 6, 3), ((1, 23, 41), 4, 2), ((1, 1, 203), 8, 1), ((1, 9, 70), 16, 2)])
def test_reconstruct_blocks_equals_the_walk_over_single_blocks(dtype, dims, B, ndim):
    """random selections (runs of every kind side by side), codes, coefficients, listed deltas and listed values"""
    rng = np.random.default_rng(50 + dtype)
    T = np.float32 if dtype == 0 else np.float64
    n = int(np.prod(dims))
    radius = 512
    h = dict(dtype=dtype, ndim=ndim, dims=(1,) + tuple(dims), blk_edge=B, eb=1e-2, radius=radius, n=n)
    nb = tuple((d + B - 1) // B for d in dims)
    sel = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=nb, p=[0.4, 0.25, 0.35])
    coef = rng.integers(-4000, 4000, size=(int((sel == 2).sum()), 4)).astype(np.int64)
    codes = rng.integers(radius - 40, radius + 40, size=n).astype(np.uint16)
    listed = rng.choice(n, size=n // 50, replace=False)
    codes[listed] = 0
    Q = np.int32 if dtype == 0 else np.int64
    sec = dict(dout_idx=np.sort(listed[:len(listed) // 2]).astype(np.uint64), dout_val=rng.integers(-20000, 20000, size=len(listed) // 2).astype(Q),
               vout_idx=np.array([3, n - 1], dtype=np.uint64), vout_val=np.array([np.nan, np.inf], dtype=T))
    got, sel2 = szh_ref.reconstruct_blocks(h, sec, codes, side=(sel, coef))
    want = _by_definition(h, sec, codes, sel, coef)
    assert sel2 is sel and got.dtype == T
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


# ---- the stream readers that advance all units / groups in step, against the bit-by-bit ones ----
def _huffman_stream(rng, n, nsym, sym_min, esc_sym=0):
    """a chunked bit stream of n random symbols under a length-limited book of nsym symbols -> (h, sec, codes)"""
    freq = np.maximum((rng.pareto(1.2, size=nsym) * 50).astype(np.int64), 1)
    lens = szh_ref.package_merge_lengths(freq, szh_ref.SHORT_LEN)
    cw, _, _ = szh_ref.canonical_codes(lens)
    idx = rng.choice(nsym, size=n, p=freq / freq.sum())
    codes = (sym_min + idx).astype(np.uint16)
    n_chunks = (n + szh_ref.CHUNK - 1) // szh_ref.CHUNK
    words, chunkwords, subbits = [], [], []
    for c in range(n_chunks):
        bits = []
        marks = []
        for k, j in enumerate(idx[c * szh_ref.CHUNK:(c + 1) * szh_ref.CHUNK]):
            if k and k % szh_ref.UNIT == 0:
                marks.append(len(bits))
            bits.extend(int(b) for b in np.binary_repr(int(cw[j]), int(lens[j])))
        marks += [len(bits)] * (szh_ref.SUBS - 1 - len(marks))
        nw = (len(bits) + 31) >> 5
        by = np.packbits(np.array(bits + [0] * (32 * nw - len(bits)), dtype=np.uint8))
        words.append(by.view(np.uint32))
        chunkwords.append(nw)
        subbits.append(marks)
    if esc_sym:
        codes[codes == esc_sym] = 0
    h = dict(n=n, max_len=int(lens.max()), sym_min=sym_min, n_chunks=n_chunks, esc_sym=esc_sym)
    sec = dict(lens=lens.astype(np.uint8), chunkwords=np.array(chunkwords, dtype=np.uint16), subbits=np.array(subbits, dtype=np.uint16).reshape(n_chunks, szh_ref.SUBS - 1),
               bitstream=np.concatenate(words))
    return h, sec, codes


@pytest.mark.parametrize("n,nsym,sym_min,esc", [(5000, 40, 32750, 0), (1024, 3, 100, 0), (2049, 300, 32600, 32700), (513, 700, 32000, 0), (100, 2, 7, 0)])
def test_unit_parallel_huffman_reader_equals_the_bit_by_bit_one(n, nsym, sym_min, esc):
    rng = np.random.default_rng(n)
    h, sec, codes = _huffman_stream(rng, n, nsym, sym_min, esc)
    slow = szh_ref.huffman_decode(h, sec)
    fast = szh_ref.huffman_decode_units(h, sec)
    assert np.array_equal(slow, codes) and np.array_equal(fast, codes)
    bad = dict(sec, subbits=sec["subbits"] + (sec["subbits"] > 0))  # a restart offset one bit late
    if (sec["subbits"] > 0).any():
        with pytest.raises(ValueError):
            szh_ref.huffman_decode_units(h, bad)


def test_single_symbol_stream_has_no_bits():
    h = dict(n=700, max_len=0, sym_min=32768, n_chunks=1)
    assert np.array_equal(szh_ref.huffman_decode_units(h, {}), szh_ref.huffman_decode(h, dict(lens=np.zeros(1, np.uint8))))


def _side_section(rng, nb, ks, share, wide):
    """a side section for blocks nb = (nbz, nby, nbx): random selections, Rice-coded coefficient differences -> (bytes, sel, coef)"""
    import struct
    nblocks = int(np.prod(nb))
    sel = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=nblocks, p=[(1 - share) / 2, (1 - share) / 2, share])
    nreg = int((sel == 2).sum())
    deltas = np.stack([rng.integers(-(3 << k), (3 << k), size=nreg, endpoint=True) for k in ks], axis=1).astype(np.int64) if nreg else np.zeros((0, 4), np.int64)
    if wide and nreg:
        deltas[rng.integers(0, nreg, size=max(1, nreg // 20)), rng.integers(0, 4)] = int(rng.integers(1 << 40, 1 << 50))  # (beyond 24 << k: 64 raw bits)
        deltas[0, 1] = -(1 << 62)
    sel_bytes = ((nblocks + 3) // 4 + 7) & ~7
    packed = np.zeros(sel_bytes * 4, dtype=np.uint8)
    packed[:nblocks] = sel
    packed = (packed.reshape(-1, 4) << (2 * np.arange(4))).sum(axis=1).astype(np.uint8)
    bits, goff = [], []
    for r in range(nreg):
        if r % 64 == 0:
            goff.append(len(bits))
        for i, k in enumerate(ks):
            v = int(deltas[r, i])
            u = ((v << 1) ^ (v >> 63)) & ((1 << 64) - 1)
            qq = u >> k
            if qq < 24:
                bits += [1] * qq + [0] + [int(b) for b in np.binary_repr(u & ((1 << k) - 1), k)][:k]
            else:
                bits += [1] * 24 + [int(b) for b in np.binary_repr(u, 64)]
    nw = (len(bits) + 31) >> 5
    by = np.packbits(np.array(bits + [0] * (32 * nw - len(bits)), dtype=np.uint8))
    words = np.frombuffer(by.tobytes(), dtype=">u4").astype(np.uint32)
    side = struct.pack("<IIQQ", 1, 2, nblocks, nreg) + packed.tobytes() + bytes(ks) + struct.pack("<I", len(goff)) \
        + np.array(goff, dtype=np.uint32).tobytes() + words.tobytes()
    return side, sel.reshape(nb), np.cumsum(deltas, axis=0)


@pytest.mark.parametrize("nb,ks,share,wide", [((3, 5, 7), (2, 3, 4, 9), 0.5, False), ((1, 1, 1000), (0, 1, 5, 12), 0.3, True), ((1, 9, 40), (7, 7, 0, 20), 0.9, True),
                                              ((2, 2, 2), (1, 1, 1, 1), 0.0, False), ((1, 1, 64), (3, 3, 3, 3), 1.0, False)])
def test_group_parallel_side_reader_equals_the_bit_by_bit_one(nb, ks, share, wide):
    rng = np.random.default_rng(sum(nb))
    B = 4
    side, sel, coef = _side_section(rng, nb, ks, share, wide)
    h = dict(blk_edge=B, ndim=3, dims=(1,) + tuple(n * B - 1 for n in nb))
    sec = dict(side=np.frombuffer(side, dtype=np.uint8))
    s1, c1 = szh_ref.parse_side(h, sec)
    s2, c2 = szh_ref.parse_side_groups(h, sec)
    assert np.array_equal(s1, sel) and np.array_equal(c1, coef)
    assert np.array_equal(s2, sel) and np.array_equal(c2, coef) and c2.dtype == np.int64
