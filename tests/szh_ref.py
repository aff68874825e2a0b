"""numpy model of the SZH1 device payload (sz3_amd/csrc/sz3hip_format.h) — TEST INFRASTRUCTURE.

Used by the GPU tests to localise faults stage by stage: expected dual-quantisation codes, payload parsing, a slow
pure-python canonical-Huffman decoder and the N-d prefix-sum reconstruction. Not used by the product.
"""
import struct
import numpy as np

MAGIC = 0x31485A53
CHUNK = 1024
SUBS = 2            # units per chunk (sz3hip_format.h: SZH_SUBS); a unit starts at the chunk's start or at a restart offset
UNIT = CHUNK // SUBS
MAX_LEN = 24        # format limit; code books of <= SHORT_SYMS symbols are limited to SHORT_LEN
SHORT_SYMS, SHORT_LEN = 512, 16


def dualquant(a, eb, radius=32768, narrow=False):
    """Expected lattice indices, codes and outliers for array `a` (any ndim <= 4), exactly as K1 computes them.
    narrow: stage 1 kept one-byte codes, i.e. deltas outside [-127, 127] became delta outliers."""
    a = np.ascontiguousarray(a)
    T = a.dtype
    # lattice arithmetic in the data type (sz3hip_kernels.hip, Lattice<T>): one rounding per multiply, no FMA
    # rint through the magic number (Lattice<T> in sz3hip_devutil.h): the bit pattern of fl(fl(a * recip) + M) is C + rint(a * recip)
    # for |a * recip| <= LIM
    if T == np.float32:
        qt = np.int32
        recip = np.float32(1.0 / (2.0 * eb))
        two_eb = np.float32(2.0 * eb)
        eb_lo = np.float32(eb)
        if float(eb_lo) > eb:
            eb_lo = np.nextafter(eb_lo, np.float32(0))
        magic, cbits, lim = np.float32(12582912.0), 0x4B400000, 1 << 22
    else:
        qt = np.int64
        recip = 1.0 / (2.0 * eb)
        two_eb = 2.0 * eb
        eb_lo = eb
        magic, cbits, lim = np.float64(6755399441055744.0), 0x4338000000000000, 1 << 51
    with np.errstate(invalid="ignore", over="ignore"):
        s = (a * recip).astype(T)
        tm = (s + magic).astype(T)
        valid = np.abs(s) <= T.type(lim)  # (False for NaN): beyond the lattice, Inf and NaN take q = 0
        q = np.where(valid, tm.view(qt) - cbits, 0).astype(qt)
        r = q.astype(T)
        dec = r * two_eb
        diff = np.abs(dec - a)
        bad = ~(diff <= eb_lo)
    # N-d Lorenzo = successive first differences with zero halo, wrap-around integer arithmetic
    d = q
    for ax in range(a.ndim):
        sl_hi = [slice(None)] * a.ndim
        sl_lo = [slice(None)] * a.ndim
        sl_hi[ax] = slice(1, None)
        sl_lo[ax] = slice(0, -1)
        nd = d.copy()  # (the first element along the axis keeps its value: the halo is zero)
        nd[tuple(sl_hi)] -= d[tuple(sl_lo)]
        d = nd
    inr = ((d >= -127) & (d <= 127)) if narrow else ((d > -radius) & (d < radius))
    codes = np.where(inr, d + radius, 0).astype(np.uint16)
    return q, d, codes, bad, ~inr


def parse(payload):
    b = bytes(payload)
    (magic, version, dtype, ndim, qbytes, predictor, radius) = struct.unpack_from("<IIBBBBI", b, 0)
    dims = struct.unpack_from("<4Q", b, 16)
    eb, n, chunk_syms, max_len, n_chunks, sym_min, sym_count, n_vout, n_dout, words, pbytes, side_bytes = struct.unpack_from(
        "<dQIIQIIQQQQQ", b, 48)
    blk_edge, blk_mask = struct.unpack_from("<II", b, 144)  # (interp_id, interp_dir: block edge / predictor mask when predictor == 2)
    (anchor_stride,) = struct.unpack_from("<Q", b, 152)       # predictor 0: the symbol that stands for a listed delta (0: symbol 0 itself; sampled books, round 6)
    h = dict(magic=magic, version=version, dtype=dtype, ndim=ndim, qbytes=qbytes, radius=radius, dims=dims, eb=eb, n=n,
             chunk_syms=chunk_syms, max_len=max_len, n_chunks=n_chunks, sym_min=sym_min, sym_count=sym_count,
             n_vout=n_vout, n_dout=n_dout, bitstream_words=words, payload_bytes=pbytes, predictor=predictor,
             side_bytes=side_bytes if predictor == 2 else 0, blk_edge=blk_edge, blk_mask=blk_mask,
             esc_sym=anchor_stride if predictor == 0 else 0)
    a16 = lambda x: (x + 15) & ~15
    tsz = 4 if dtype == 0 else 8
    off = 160
    o = {}
    o["lens"] = off
    off = a16(off + sym_count)
    o["chunkwords"] = off
    off = a16(off + 2 * n_chunks)
    o["subbits"] = off  # (format 4) bit offset of a chunk's symbol 512: the decoder's restart point
    off = a16(off + 2 * (SUBS - 1) * n_chunks)
    o["vout_idx"] = off
    off += 8 * n_vout
    o["vout_val"] = off
    off = a16(off + tsz * n_vout)
    o["dout_idx"] = off
    off += 8 * n_dout
    o["dout_val"] = off
    off = a16(off + qbytes * n_dout)
    o["side"] = off
    off = a16(off + h["side_bytes"])
    o["bitstream"] = off
    o["end"] = off + 4 * words
    T = np.float32 if dtype == 0 else np.float64
    Q = np.int32 if dtype == 0 else np.int64
    buf = np.frombuffer(b, dtype=np.uint8)
    sec = dict(
        lens=buf[o["lens"]:o["lens"] + sym_count].copy(),
        chunkwords=np.frombuffer(b, dtype=np.uint16, count=n_chunks, offset=o["chunkwords"]).copy(),
        subbits=np.frombuffer(b, dtype=np.uint16, count=(SUBS - 1) * n_chunks, offset=o["subbits"]).copy().reshape(n_chunks, SUBS - 1),
        vout_idx=np.frombuffer(b, dtype=np.uint64, count=n_vout, offset=o["vout_idx"]).copy(),
        vout_val=np.frombuffer(b, dtype=T, count=n_vout, offset=o["vout_val"]).copy(),
        dout_idx=np.frombuffer(b, dtype=np.uint64, count=n_dout, offset=o["dout_idx"]).copy(),
        dout_val=np.frombuffer(b, dtype=Q, count=n_dout, offset=o["dout_val"]).copy(),
        bitstream=np.frombuffer(b, dtype=np.uint32, count=words, offset=o["bitstream"]).copy(),
        side=buf[o["side"]:o["side"] + h["side_bytes"]].copy(),
    )
    return h, o, sec


def canonical_codes(lens):
    """(code, len) per symbol index from code lengths; canonical order = (len, symbol)."""
    lens = np.asarray(lens, dtype=np.int64)
    cnt = np.bincount(lens, minlength=MAX_LEN + 2)
    cnt[0] = 0
    first = np.zeros(MAX_LEN + 2, dtype=np.int64)
    code = 0
    for l in range(1, MAX_LEN + 1):
        code = (code + (cnt[l - 1] if l > 1 else 0)) << (1 if l > 1 else 0)
        first[l] = code
    nxt = first.copy()
    codes = np.zeros(len(lens), dtype=np.int64)
    for i, l in enumerate(lens):
        if l:
            codes[i] = nxt[l]
            nxt[l] += 1
    return codes, first, cnt


BOOK_MARGIN = 8
SMALL_SYMS = 256


def book_symbols(present):
    """-> (set of symbols a stream's code book has code words for, margins applied?) given the sorted symbols that occur.
    Small alphabets (sz3hip_kernels.hip, cb_margins): every symbol from 8 below the smallest to 8 above the largest one, the empty
    bins counted once — unless symbol 0 occurs, a single symbol occurs, or the widened range exceeds the small path's 256 symbols."""
    present = np.asarray(present).astype(np.int64)
    if len(present) < 2 or len(present) > SMALL_SYMS or present.min() == 0:
        return set(present.tolist()), False
    lo2, hi2 = max(int(present.min()) - BOOK_MARGIN, 1), min(int(present.max()) + BOOK_MARGIN, 65535)
    if hi2 - lo2 + 1 > SMALL_SYMS:
        return set(present.tolist()), False
    return set(range(lo2, hi2 + 1)), True


def book_histogram(freq, sym_min):
    """-> (counts the code book is built from, their first symbol, the book's length limit) for a stream whose symbols sym_min + i occur
    freq[i] times: book_symbols' widened range with every empty bin counted once where the margins apply, else the counts as they are"""
    freq = np.asarray(freq, dtype=np.int64)
    present = sym_min + np.nonzero(freq)[0]
    book, filled = book_symbols(present)
    if filled:
        lo, hi = min(book), max(book)
        wide = np.ones(hi - lo + 1, dtype=np.int64)
        wide[sym_min - lo:sym_min - lo + len(freq)] = np.maximum(freq, 1)
        freq, sym_min = wide, lo
    return freq, sym_min, SHORT_LEN if len(book) <= SHORT_SYMS else MAX_LEN


def kraft(lens):
    lens = np.asarray(lens, dtype=np.int64)
    return float(np.sum(2.0 ** (-lens[lens > 0].astype(np.float64))))


def huffman_cost(freq):
    """-> (total bits, tree height) of an unlimited Huffman code over the non-zero counts of `freq` (heapq: independent of the kernels)"""
    import heapq
    heap = [(int(f), i, 0) for i, f in enumerate(freq) if f]   # (freq, tiebreak, height)
    heapq.heapify(heap)
    cost = 0
    cnt = len(freq)
    while len(heap) > 1:
        f1, _, h1 = heapq.heappop(heap)
        f2, _, h2 = heapq.heappop(heap)
        cost += f1 + f2
        cnt += 1
        heapq.heappush(heap, (f1 + f2, cnt, max(h1, h2) + 1))
    return cost, heap[0][2]


def assert_book_optimal(freq, lens, limit):
    """the book's total bits over `freq` equal an unlimited Huffman code's when that code respects the length limit (16 bits up to
    512 symbols, else 24), otherwise lie within 0.2 % of it (length-limited code; package_merge_lengths, the optimum under the limit,
    stays within 0.06 % on every crafted family of tests/crafted_codes.py)"""
    cost, height = huffman_cost(freq)
    gpu_cost = int((np.asarray(freq, dtype=np.int64) * np.asarray(lens).astype(np.int64)).sum())
    if height <= limit:
        assert gpu_cost == cost, "code is not optimal"
    else:
        assert cost <= gpu_cost <= cost * 1.002, "length-limited code too far from optimal"


def package_merge_lengths(freq, limit):
    """-> code length per entry of `freq` (0 where the count is 0) of an optimal prefix code whose longest word has at most `limit`
    bits: package-merge (Larmore & Hirschberg 1990) in its boundary form. Level by level, deepest first, the leaves are merged with
    the packages (pairs) of the level below; the cheapest 2m - 2 items of the top level are the solution, and a leaf's length is the
    number of levels at which it was taken. Exact integer arithmetic; no code with words of at most `limit` bits costs less.
    A single symbol gets one bit (the format itself stores no bits for such a stream)."""
    freq = np.asarray(freq, dtype=np.int64)
    lens = np.zeros(len(freq), dtype=np.int64)
    idx = np.nonzero(freq)[0]
    m = len(idx)
    if m == 0:
        return lens
    if m == 1:
        lens[idx] = 1
        return lens
    if (1 << limit) < m:
        raise ValueError("%d symbols have no prefix code of %d bits" % (m, limit))
    order = idx[np.argsort(freq[idx], kind="stable")]
    w = freq[order]
    is_leaf = []                       # per level: the merged list's flags, cheapest first (leaves before packages of equal weight)
    packages = np.zeros(0, dtype=np.int64)
    for _ in range(limit):
        both = np.concatenate([w, packages])
        perm = np.argsort(both, kind="stable")
        merged = both[perm]
        is_leaf.append(perm < m)
        pairs = len(merged) // 2
        packages = merged[0:2 * pairs:2] + merged[1:2 * pairs:2]
    take = 2 * m - 2
    sorted_lens = np.zeros(m, dtype=np.int64)
    for flags in reversed(is_leaf):
        leaves = int(np.count_nonzero(flags[:take]))
        sorted_lens[:leaves] += 1      # the leaves taken at a level are its cheapest ones
        take = 2 * (take - leaves)     # every package taken stands for two items of the level below
    lens[order] = sorted_lens
    return lens


def chunk_table(codes, lens, sym_min, esc_sym=0):
    """-> (bits, chunkwords, subbits) per chunk that a stream of `codes` must have under the code lengths `lens` (the payload's table,
    first entry symbol sym_min): the chunk's bit count, its count of 32-bit words, and the bit offsets of its later units (the sum over
    the symbols in front of the unit; a ragged last chunk that ends before a unit's start has the chunk's whole bit count there).
    esc_sym: the symbol whose code word stands for code 0 (sampled books)."""
    codes = np.asarray(codes).reshape(-1)
    n = codes.size
    table = np.zeros(65536, dtype=np.int64)
    table[sym_min:sym_min + len(lens)] = np.asarray(lens, dtype=np.int64)
    if esc_sym:
        table[0] = table[esc_sym]
    n_chunks = (n + CHUNK - 1) // CHUNK
    per = np.zeros(n_chunks * CHUNK, dtype=np.int64)
    per[:n] = table[codes]
    units = per.reshape(n_chunks, SUBS, UNIT).sum(axis=2)
    run = np.cumsum(units, axis=1)
    bits = run[:, -1]
    return bits, (bits + 31) >> 5, run[:, :-1]


def huffman_decode(h, sec, chunks=None):
    """slow reference decoder of the chunked bit-stream -> uint16 codes. chunks: the chunks to decode (default: all of them); the
    other chunks' elements stay 0."""
    n = h["n"]
    out = np.zeros(n, dtype=np.uint16)
    lens = sec["lens"]
    if h["max_len"] == 0:
        out[:] = h["sym_min"]
        return out
    codes, _, _ = canonical_codes(lens)
    table = {}
    for i, l in enumerate(lens):
        if l:
            sym = h["sym_min"] + i
            table[(int(l), int(codes[i]))] = 0 if (h.get("esc_sym") and sym == h["esc_sym"]) else sym  # (the escape symbol decodes as symbol 0)
    offs = np.concatenate([[0], np.cumsum(sec["chunkwords"].astype(np.int64))])
    bs = sec["bitstream"]
    for c in (range(h["n_chunks"]) if chunks is None else chunks):
        c = int(c)
        words = bs[offs[c]:offs[c + 1]]
        bits = np.unpackbits(words.view(np.uint8)) if len(words) else np.zeros(0, np.uint8)  # bytes are in stream order
        s0 = c * CHUNK
        ns = min(CHUNK, n - s0)
        pos = 0
        for i in range(ns):
            if i and i % UNIT == 0 and int(sec["subbits"][c][i // UNIT - 1]) != pos:
                raise ValueError("restart offset %d of chunk %d is %d, the symbol starts at bit %d" % (i // UNIT, c, sec["subbits"][c][i // UNIT - 1], pos))
            v = 0
            l = 0
            while True:
                v = (v << 1) | int(bits[pos])
                pos += 1
                l += 1
                sym = table.get((l, v))
                if sym is not None:
                    out[s0 + i] = sym
                    break
                if l > MAX_LEN:
                    raise ValueError("bad code in chunk %d" % c)
    return out


def reconstruct(h, sec, codes):
    T = np.float32 if h["dtype"] == 0 else np.float64
    Q = np.int32 if h["dtype"] == 0 else np.int64
    d = np.where(codes == 0, 0, codes.astype(np.int64) - h["radius"]).astype(Q)
    d[sec["dout_idx"].astype(np.int64)] = sec["dout_val"]
    q = d.reshape(h["dims"])
    for ax in range(4):
        if q.shape[ax] > 1:  # (a sum along an extent of one is the array itself)
            with np.errstate(over="ignore"):
                q = np.cumsum(q, axis=ax, dtype=Q)
    x = (q.astype(T) * T(2.0 * h["eb"])).reshape(-1)
    x[sec["vout_idx"].astype(np.int64)] = sec["vout_val"]
    return x


def decode_payload(payload):
    h, o, sec = parse(payload)
    codes = huffman_decode(h, sec)
    return reconstruct(h, sec, codes), h


# ---- block-composed predictor (predictor id 2, sz3hip_regress.hip): side section and a slow block-by-block decoder ----
def parse_side(h, sec):
    """-> (selection per block uint8 [nbz, nby, nbx], coefficient lattice values int64 [n_reg, 4] in block raster order)"""
    side = sec["side"].tobytes()
    coding, sel_bits, nblocks, nreg = struct.unpack_from("<IIQQ", side, 0)
    B = h["blk_edge"]
    four = h["ndim"] == 4  # (round 4: 4-D arrays — the slowest extent in dims[0], five coefficients per regression block)
    nc, pb = (5, 16) if four else (4, 8)
    nb = [(d + B - 1) // B for d in (h["dims"] if four else h["dims"][1:])]
    assert coding == 1 and sel_bits == 2 and nblocks == int(np.prod(nb))
    sel_bytes = ((nblocks + 3) // 4 + 7) & ~7
    packed = np.frombuffer(side, dtype=np.uint8, count=sel_bytes, offset=24)
    sel = ((packed[:, None] >> (2 * np.arange(4))) & 3).reshape(-1)[:nblocks].astype(np.uint8)
    # Rice-coded differences: [u8 k[nc], padding][u32 groups] (8 bytes, 16 for 4-D arrays) [u32 bit offset per group of 64 blocks][u32 words, MSB first]
    p0 = 24 + sel_bytes
    ks = list(side[p0:p0 + nc])
    ngroups, = struct.unpack_from("<I", side, p0 + pb - 4)
    assert ngroups == (nreg + 63) // 64
    goff = np.frombuffer(side, dtype=np.uint32, count=ngroups, offset=p0 + pb)
    words = np.frombuffer(side, dtype=np.uint32, offset=p0 + pb + 4 * ngroups)
    bits = np.unpackbits(words.astype(">u4").view(np.uint8))
    deltas = np.zeros((nreg, nc), dtype=np.int64)
    for g in range(ngroups):
        pos = int(goff[g])
        for r in range(g * 64, min(nreg, (g + 1) * 64)):
            for i in range(nc):
                q = 0
                while q < 24 and bits[pos]:
                    q += 1
                    pos += 1
                if q < 24:
                    pos += 1
                    low = 0
                    for _ in range(ks[i]):
                        low = (low << 1) | int(bits[pos])
                        pos += 1
                    u = (q << ks[i]) | low
                else:
                    u = 0
                    for _ in range(64):
                        u = (u << 1) | int(bits[pos])
                        pos += 1
                deltas[r, i] = (u >> 1) ^ -(u & 1)
    coef = np.cumsum(deltas, axis=0)
    assert int((sel == 2).sum()) == nreg
    return sel.reshape(nb), coef


def reconstruct_blocks4(h, sec, codes):
    """the same for a 4-D array: blocks of B^4, first-order Lorenzo (fifteen neighbours) or regression with five coefficients"""
    import itertools
    T = np.float32 if h["dtype"] == 0 else np.float64
    dims = list(h["dims"])
    B, eb, radius = h["blk_edge"], h["eb"], h["radius"]
    sel, coef = parse_side(h, sec)
    dflat = np.where(codes == 0, 0, codes.astype(np.int64) - radius).astype(np.int64)
    dflat[sec["dout_idx"].astype(np.int64)] = sec["dout_val"]
    q = np.zeros([d + 1 for d in dims], dtype=np.int64)  # a zero halo layer on the low side
    out = np.zeros(dims, dtype=T)
    recip = T(1.0 / (2.0 * eb)) if T == np.float32 else 1.0 / (2.0 * eb)
    lim = T(8388608.0) if T == np.float32 else 4503599627370496.0
    step_ind, step_lin = 2.0 * (eb / 5), 2.0 * (eb / 5 / B)
    signs = [(o, -1 if sum(o) % 2 else 1) for o in itertools.product((0, 1), repeat=4) if any(o)]
    pos, r = 0, 0
    for bw, bz, by, bx in itertools.product(*[range(n) for n in sel.shape]):
        o = [bw * B, bz * B, by * B, bx * B]
        e = [min(B, dims[i] - o[i]) for i in range(4)]
        m = int(np.prod(e))
        sl = tuple(slice(o[i], o[i] + e[i]) for i in range(4))
        if int(sel[bw, bz, by, bx]) == 2:
            lc = coef[r]
            r += 1
            rc = [T(float(lc[i]) * step_lin) for i in range(4)] + [T(float(lc[4]) * step_ind)]
            idx = np.meshgrid(*[np.arange(n) for n in e], indexing="ij")
            pred = (rc[0] * idx[0].astype(T)).astype(T)
            for i in (1, 2, 3):
                pred = (pred + (rc[i] * idx[i].astype(T)).astype(T)).astype(T)
            pred = (pred + rc[4]).astype(T)
            cc = codes[pos:pos + m].reshape(e).astype(np.int64)
            val = (pred.astype(np.float64) + (2 * (cc - radius)).astype(np.float64) * eb).astype(T)
            with np.errstate(invalid="ignore", over="ignore"):
                sc = val * recip
                ok = np.abs(sc) < lim
                rr = np.rint(np.where(ok, sc, 0)).astype(T)
                bad = ~ok | ~(np.abs(rr * T(2.0 * eb) - val) <= (T(eb) if float(T(eb)) <= eb else np.nextafter(T(eb), T(0))))
            q[tuple(slice(o[i] + 1, o[i] + 1 + e[i]) for i in range(4))] = np.where((cc == 0) | bad, 0, rr.astype(np.int64))
            out[sl] = np.where(cc == 0, 0, val)
        else:
            d = dflat[pos:pos + m].reshape(e)
            for i0, i1, i2, i3 in itertools.product(*[range(n) for n in e]):
                c = (o[0] + i0 + 1, o[1] + i1 + 1, o[2] + i2 + 1, o[3] + i3 + 1)
                acc = int(d[i0, i1, i2, i3])
                for off, sg in signs:  # delta = sum over the 16 corners of (-1)^|off| q: the fifteen others go to the other side
                    acc -= sg * int(q[c[0] - off[0], c[1] - off[1], c[2] - off[2], c[3] - off[3]])
                q[c] = acc
            out[sl] = q[tuple(slice(o[i] + 1, o[i] + 1 + e[i]) for i in range(4))].astype(T) * T(2.0 * eb)
        pos += m
    x = out.reshape(-1)
    x[sec["vout_idx"].astype(np.int64)] = sec["vout_val"]
    return x, sel


def lorenzo_block_elementwise(q, delta, origin, extents, order):
    """THE DEFINITION of a Lorenzo block's inverse. q: the lattice array with two zero halo layers on the low side of every axis
    (int64, element (z, y, x) at q[z + 2, y + 2, x + 2]), filled in place for the block at `origin` = (z0, y0, x0) with `extents` =
    (ez, ey, ex); delta: the block's residuals [ez, ey, ex]; order 1 / 2: the stencil (1, -1) / (1, -2, 1) per axis. Element by
    element in raster order, in Python integers: q = delta - sum over the stencil's other corners of w_a w_b w_c q[z - a, y - b, x - c]."""
    w = (1, -1) if order == 1 else (1, -2, 1)
    m = len(w) - 1
    (z0, y0, x0), (ez, ey, ex) = origin, extents
    for k in range(ez):
        for j in range(ey):
            for i in range(ex):
                z, y, x = z0 + k + 2, y0 + j + 2, x0 + i + 2
                acc = int(delta[k, j, i])
                for a in range(m + 1):
                    for b_ in range(m + 1):
                        for c_ in range(m + 1):
                            if a or b_ or c_:
                                acc -= w[a] * w[b_] * w[c_] * int(q[z - a, y - b_, x - c_])
                q[z, y, x] = acc


def lorenzo_block(q, delta, origin, extents, order):
    """the same block at once, exact in int64 (tests/test_block_model_cpu.py holds the two forms equal): the block with its low-side
    halo of `order` layers in a box of extents + order whose interior is zeroed; the box's own Lorenzo residuals by differencing
    along each axis `order` times (a halo position's residual reads halo positions only: the zeroed interior does not reach it);
    the interior's residuals replaced by the block's; back by cumulative sums along each axis, `order` times. What holds for a block
    holds for any box of elements that obey one recurrence: reconstruct_blocks hands a run of blocks of one order along x over as one."""
    m = order
    (z0, y0, x0), (ez, ey, ex) = origin, extents
    src = q[z0 + 2 - m:z0 + 2 + ez, y0 + 2 - m:y0 + 2 + ey, x0 + 2 - m:x0 + 2 + ex]
    box = src.astype(np.int64)  # (a copy)
    box[m:, m:, m:] = 0
    for ax in range(3):
        hi = tuple(slice(1, None) if a == ax else slice(None) for a in range(3))
        lo = tuple(slice(0, -1) if a == ax else slice(None) for a in range(3))
        for _ in range(m):
            box[hi] -= box[lo].copy()
    box[m:, m:, m:] = delta
    for ax in range(3):
        for _ in range(m):
            np.cumsum(box, axis=ax, out=box)
    src[m:, m:, m:] = box[m:, m:, m:]


def _lattice_of(val, cc, eb, T):
    """the lattice values a regression block leaves for its neighbours: rint(val / 2 eb), 0 where the code is 0 or the value does not
    sit on the lattice within the bound"""
    recip = T(1.0 / (2.0 * eb)) if T == np.float32 else 1.0 / (2.0 * eb)
    lim = T(8388608.0) if T == np.float32 else 4503599627370496.0
    with np.errstate(invalid="ignore", over="ignore"):
        sc = val * recip
        ok = np.abs(sc) < lim
        rr = np.rint(np.where(ok, sc, 0)).astype(T)
        bad = ~ok | ~(np.abs(rr * T(2.0 * eb) - val) <= (T(eb) if float(T(eb)) <= eb else np.nextafter(T(eb), T(0))))
    return np.where((cc == 0) | bad, 0, rr.astype(np.int64))


def regression_block(cc, lc, B, eb, radius, T, nd1):
    """THE DEFINITION of a regression block: cc its codes [ez, ey, ex] (int64), lc its four coefficient lattice values ->
    (lattice values for the neighbours, output values): pred + 2 (code - radius) eb, pred = c0 z + c1 y + c2 x + c3 in T"""
    ez, ey, ex = cc.shape
    step_ind, step_lin = 2.0 * (eb / nd1), 2.0 * (eb / nd1 / B)
    rc = [T(float(lc[i]) * step_lin) for i in range(3)] + [T(float(lc[3]) * step_ind)]
    i0, i1, i2 = np.meshgrid(np.arange(ez), np.arange(ey), np.arange(ex), indexing="ij")
    pred = (rc[0] * i0.astype(T) + rc[1] * i1.astype(T) + rc[2] * i2.astype(T) + rc[3]).astype(T)
    val = (pred.astype(np.float64) + (2 * (cc - radius)).astype(np.float64) * eb).astype(T)
    return _lattice_of(val, cc, eb, T), np.where(cc == 0, 0, val)


def regression_run(cc, lcs, B, eb, radius, T, nd1):
    """a run of regression blocks along x at once (tests/test_block_model_cpu.py holds it equal to regression_block block by block):
    cc the run's codes [ez, ey, ex of the run], lcs [blocks of the run, 4]; the same operations in T, element by element"""
    ez, ey, ex = cc.shape
    step_ind, step_lin = 2.0 * (eb / nd1), 2.0 * (eb / nd1 / B)
    lcs = np.asarray(lcs, dtype=np.int64)
    bi = np.arange(ex) // B
    rc = [(lcs[:, i].astype(np.float64) * step_lin).astype(T)[bi] for i in range(3)] + [(lcs[:, 3].astype(np.float64) * step_ind).astype(T)[bi]]
    i0 = np.arange(ez).astype(T)[:, None, None]
    i1 = np.arange(ey).astype(T)[None, :, None]
    i2 = (np.arange(ex) % B).astype(T)[None, None, :]
    pred = (rc[0][None, None, :] * i0 + rc[1][None, None, :] * i1 + rc[2][None, None, :] * i2 + rc[3][None, None, :]).astype(T)
    val = (pred.astype(np.float64) + (2 * (cc - radius)).astype(np.float64) * eb).astype(T)
    return _lattice_of(val, cc, eb, T), np.where(cc == 0, 0, val)


def block_positions(dims3, B):
    """-> int64 [dz, dy, dx]: the position in the code stream of every element (blocks in raster order, raster order inside a block)"""
    n = [np.arange(d) for d in dims3]
    b = [v // B for v in n]                                   # block index per coordinate
    l = [v % B for v in n]                                    # local index
    e = [np.minimum(B, d - np.arange((d + B - 1) // B) * B) for d in dims3]  # block extents per block index
    size = e[0][:, None, None] * e[1][None, :, None] * e[2][None, None, :]
    start = (np.cumsum(size.reshape(-1)) - size.reshape(-1)).reshape(size.shape)
    ey, ex = e[1][b[1]], e[2][b[2]]
    return (start[b[0][:, None, None], b[1][None, :, None], b[2][None, None, :]]
            + (l[0][:, None, None] * ey[None, :, None] + l[1][None, :, None]) * ex[None, None, :] + l[2][None, None, :]).astype(np.int64)


def reconstruct_blocks(h, sec, codes, side=None):
    """numpy model of the block decoder: blocks in raster order (any order that respects the low-side dependencies works),
    Lorenzo blocks invert their integer stencil (lorenzo_block), regression blocks are pred + 2*(code - radius)*eb (regression_run);
    a run of blocks of one kind along x is taken at once. side: parse_side's result where the caller has it already."""
    if h["ndim"] == 4:
        return reconstruct_blocks4(h, sec, codes)
    T = np.float32 if h["dtype"] == 0 else np.float64
    dz, dy, dx = h["dims"][1:]
    B, eb, radius = h["blk_edge"], h["eb"], h["radius"]
    sel, coef = side if side is not None else parse_side(h, sec)
    codes = np.asarray(codes)
    dflat = np.where(codes == 0, 0, codes.astype(np.int64) - radius).astype(np.int64)
    dflat[sec["dout_idx"].astype(np.int64)] = sec["dout_val"]  # (outlier indices are code positions)
    # the codes are stored block by block (block raster order, raster order inside a block): back to element order
    pos = block_positions((dz, dy, dx), B)
    d = dflat[pos]
    c3 = codes[pos].astype(np.int64)
    del pos
    q = np.zeros((dz + 2, dy + 2, dx + 2), dtype=np.int64)  # two zero halo layers on the low side
    out = np.zeros((dz, dy, dx), dtype=T)
    nd1 = h["ndim"] + 1  # (1-D / 2-D arrays are seen as (1, 1, n) / (1, dy, dx): RegressionPredictor.hpp:22-26 divides by N + 1)
    two_eb = T(2.0 * eb)
    nreg_before = np.concatenate([[0], np.cumsum(sel.reshape(-1) == 2)])  # (regression blocks in front of a block, raster order)
    nbx = sel.shape[2]
    for bz in range(sel.shape[0]):
        for by in range(sel.shape[1]):
            z0, y0 = bz * B, by * B
            ez, ey = min(B, dz - z0), min(B, dy - y0)
            row = sel[bz, by]
            cut = np.flatnonzero(row[1:] != row[:-1]) + 1
            for b0, b1 in zip(np.concatenate([[0], cut]).tolist(), np.concatenate([cut, [nbx]]).tolist()):
                s = int(row[b0])
                x0 = b0 * B
                ex = min(b1 * B, dx) - x0
                blk = (slice(z0, z0 + ez), slice(y0, y0 + ey), slice(x0, x0 + ex))
                if s == 2:
                    r = int(nreg_before[(bz * sel.shape[1] + by) * nbx + b0])
                    qt, val = regression_run(c3[blk], coef[r:r + (b1 - b0)], B, eb, radius, T, nd1)
                    q[z0 + 2:z0 + 2 + ez, y0 + 2:y0 + 2 + ey, x0 + 2:x0 + 2 + ex] = qt
                    out[blk] = val
                else:
                    lorenzo_block(q, d[blk], (z0, y0, x0), (ez, ey, ex), s + 1)
                    out[blk] = q[z0 + 2:z0 + 2 + ez, y0 + 2:y0 + 2 + ey, x0 + 2:x0 + 2 + ex].astype(T) * two_eb
    x = out.reshape(-1)
    x[sec["vout_idx"].astype(np.int64)] = sec["vout_val"]
    return x, sel


# ---- the same streams read a unit / a group of blocks at a time, for arrays of millions of values ----
def huffman_decode_units(h, sec):
    """huffman_decode's codes (tests/test_block_model_cpu.py holds the two equal), every unit of the stream advanced in step: a unit
    starts at its chunk's first word or at the chunk's restart offset, and a table of 2^(longest word) entries reads a symbol at a time.
    Checks that a unit ends where the chunk's next one starts."""
    n = h["n"]
    if h["max_len"] == 0:
        return np.full(n, h["sym_min"], dtype=np.uint16)
    lens = sec["lens"].astype(np.int64)
    L = int(lens.max())
    order = np.lexsort((np.arange(len(lens)), lens))  # canonical order: (len, symbol)
    order = order[lens[order] > 0]
    syms = (h["sym_min"] + order).astype(np.int64)
    if h.get("esc_sym"):
        syms[syms == h["esc_sym"]] = 0
    span = 1 << (L - lens[order])
    assert int(span.sum()) <= 1 << L, "the lengths are no prefix code"
    t_sym = np.zeros(1 << L, dtype=np.uint16)
    t_len = np.zeros(1 << L, dtype=np.int64)    # (0: no code word starts like this)
    t_sym[:int(span.sum())] = np.repeat(syms, span)
    t_len[:int(span.sum())] = np.repeat(lens[order], span)
    n_chunks = h["n_chunks"]
    offs = np.concatenate([[0], np.cumsum(sec["chunkwords"].astype(np.int64))])
    data = np.concatenate([sec["bitstream"].view(np.uint8), np.zeros(8, np.uint8)]).astype(np.int64)  # bytes are in stream order
    start = np.zeros((n_chunks, SUBS), dtype=np.int64)
    start[:, 1:] = sec["subbits"].astype(np.int64)
    pos = (32 * offs[:-1, None] + start).reshape(-1)
    first = pos.copy()
    count = np.clip(n - np.arange(n_chunks * SUBS, dtype=np.int64) * UNIT, 0, UNIT)
    out = np.zeros(n_chunks * CHUNK, dtype=np.uint16)
    base = np.arange(n_chunks * SUBS, dtype=np.int64) * UNIT
    for i in range(UNIT):
        act = np.flatnonzero(count > i)
        if not act.size:
            break
        p = pos[act]
        by = p >> 3
        v = (data[by] << 24) | (data[by + 1] << 16) | (data[by + 2] << 8) | data[by + 3]
        win = (v >> (32 - L - (p & 7))) & ((1 << L) - 1)
        l = t_len[win]
        if not l.all():
            raise ValueError("bad code in unit %d" % int(act[np.flatnonzero(l == 0)[0]]))
        out[base[act] + i] = t_sym[win]
        pos[act] = p + l
    ends = pos.reshape(n_chunks, SUBS)
    if not np.array_equal(ends[:, :-1] - first.reshape(n_chunks, SUBS)[:, :1], start[:, 1:]):
        raise ValueError("a restart offset is not where its unit's first symbol starts")
    if not np.array_equal((ends[:, -1] - 32 * offs[:-1] + 31) >> 5, sec["chunkwords"].astype(np.int64)):
        raise ValueError("a chunk's word count is not its bits' count")
    return out[:n]


def parse_side_groups(h, sec):
    """parse_side's result (tests/test_block_model_cpu.py holds the two equal), the groups of 64 regression blocks advanced in step"""
    side = sec["side"].tobytes()
    coding, sel_bits, nblocks, nreg = struct.unpack_from("<IIQQ", side, 0)
    B = h["blk_edge"]
    four = h["ndim"] == 4
    nc, pb = (5, 16) if four else (4, 8)
    nb = [(d + B - 1) // B for d in (h["dims"] if four else h["dims"][1:])]
    assert coding == 1 and sel_bits == 2 and nblocks == int(np.prod(nb))
    sel_bytes = ((nblocks + 3) // 4 + 7) & ~7
    packed = np.frombuffer(side, dtype=np.uint8, count=sel_bytes, offset=24)
    sel = ((packed[:, None] >> (2 * np.arange(4))) & 3).reshape(-1)[:nblocks].astype(np.uint8)
    p0 = 24 + sel_bytes
    ks = list(side[p0:p0 + nc])
    ngroups, = struct.unpack_from("<I", side, p0 + pb - 4)
    assert ngroups == (nreg + 63) // 64 and max(ks, default=0) <= 56
    goff = np.frombuffer(side, dtype=np.uint32, count=ngroups, offset=p0 + pb).astype(np.int64)
    words = np.frombuffer(side, dtype=np.uint32, offset=p0 + pb + 4 * ngroups)
    data = np.concatenate([words.astype(">u4").view(np.uint8), np.zeros(16, np.uint8)]).astype(np.uint64)  # MSB first

    def window(p):  # the 64 bits from bit p on, left-aligned
        by = (p >> 3).astype(np.int64)
        sh = (p & 7).astype(np.uint64)
        w = np.zeros(len(p), dtype=np.uint64)
        for k in range(8):
            w = (w << np.uint64(8)) | data[by + k]
        return (w << sh) | (data[by + 8] >> (np.uint64(8) - sh))  # (a shift by 8 of a byte: 0)

    deltas = np.zeros((ngroups * 64, nc), dtype=np.int64)
    pos = goff.copy()
    gbase = np.arange(ngroups, dtype=np.int64) * 64
    for r in range(64):
        act = np.flatnonzero(gbase + r < nreg)
        if not act.size:
            break
        for i in range(nc):
            p = pos[act]
            inv = (~(window(p) >> np.uint64(40))) & np.uint64(0xFFFFFF)   # the first 24 bits, inverted: the unary part ends at its highest set bit
            q = np.where(inv == 0, 24, 23 - np.floor(np.log2(np.maximum(inv, 1).astype(np.float64))).astype(np.int64))
            esc = q == 24
            p = p + q + np.where(esc, 0, 1)
            w = window(p)
            k = ks[i]
            low = (w >> np.uint64(64 - k)) if k else np.zeros(len(p), dtype=np.uint64)
            u = np.where(esc, w, (q.astype(np.uint64) << np.uint64(k)) | low)
            pos[act] = p + np.where(esc, 64, k)
            deltas[gbase[act] + r, i] = (u >> np.uint64(1)).astype(np.int64) ^ -((u & np.uint64(1)).astype(np.int64))
    coef = np.cumsum(deltas[:nreg], axis=0)
    assert int((sel == 2).sum()) == nreg
    return sel.reshape(nb), coef
