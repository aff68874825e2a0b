"""Arrays whose stock ALGO_NOPRED code stream is prescribed symbol by symbol — TEST INFRASTRUCTURE (no tests).

The reference's ALGO_NOPRED quantises every value against 0, so with eb a power of two x = 2 eb d codes to exactly d + radius, element by
element, in any order: the test prescribes the histogram AND the places of the symbols of the reference's own unindexed Huffman bit
stream, the one the device stage of sz3hip_stock.hip reads (k_stock_huff_sync, k_stock_huff_write, stock_decode_one) and writes
(k_stock_enc_bits, k_stock_enc_pack). The families are the streams on which that stage leaves the path smooth fields keep it on:
  * fixed-length codes whose length does not divide 4096 (equal counts over 8 or 32 symbols) never re-synchronise: every pass of the
    restart-point loop repairs one subsequence, so the pass cap and the host walk behind it are reached (sync_passes is the model);
  * fixed-length codes of 1 and 8 bits sit on every subsequence boundary: one pass, streams of whole subsequences, padding bits that
    are code words themselves;
  * chains (powers of two, Fibonacci counts) give code words beyond the decoder's 12-bit table and, at 35 Fibonacci counts, beyond
    32 bits: the decoder's window refill and the coder's third stage word.
tests/test_crafted_stock_cpu.py holds every family to its stated regime with the reference alone and keeps
tests/golden/crafted_stock.npz (the reference's containers) fresh; tests/test_gpu_crafted_stock.py shows them to the kernels."""
import functools
import heapq
import struct

import numpy as np

from crafted_codes import _fib, delta_stream, deltas_by_count

RADIUS = 32768
EB = 2.0 ** -10          # a power of two: d * 2 eb is exact in f32 and f64, and |x| / eb gives 2 |d| back exactly
SUB_BITS = 4096          # = STOCK_SUB_BITS: the decoder's subsequence
ENC_TILE = 2048          # = STOCK_ENC_TILE: symbols of one coder tile
MAX_PASSES = 12          # = STOCK_SYNC_MAX_PASSES
ROUTE_DEVICE, ROUTE_HOST_SWITCH, ROUTE_HOST_CAP, ROUTE_SINGLE = 0, 1, 2, 3


def array_from_codes(d, dtype):
    """-> (x = d * 2 EB as dtype, the codes d + 32768 the reference's ALGO_NOPRED gives x at the bound EB)"""
    d = np.asarray(d, dtype=np.int64)
    assert int(np.abs(d).max()) < RADIUS
    return (d.astype(np.float64) * (2.0 * EB)).astype(dtype), (d + RADIUS).astype(np.uint16)


def sync_passes(n, L):
    """-> (nsub, passes): the restart-point loop of szk_launch_stock_huff_decode over n code words of L bits each, with no pass cap.
    Subsequences of 4096 bits over n * L bits rounded up to whole bytes; thread i decodes from where thread i - 1 ended in the pass
    before (at first: from its own first bit) to the first code-word boundary at or beyond its bound; a code word that would run beyond
    the stream ends the walk, and the thread hands on its bound. Passes repeat until none moved anything; the count includes that
    last, still pass."""
    total = (n * L + 7) // 8 * 8
    nsub = (total + SUB_BITS - 1) // SUB_BITS
    start = [min(i * SUB_BITS, total) for i in range(nsub + 1)]
    nxt = list(start)
    last = [None] * nsub
    passes = 0
    while True:
        passes += 1
        changed = False
        for i in range(nsub):
            if last[i] == start[i]:
                continue
            last[i] = start[i]
            bound = min((i + 1) * SUB_BITS, total)
            pos = start[i]
            if pos < bound:
                pos += (bound - pos + L - 1) // L * L       # whole code words up to the first boundary at or beyond the bound
                while pos > total:                         # ... of which the stream's end cuts the last ones off
                    pos -= L
                if pos < bound:
                    pos = bound
            if nxt[i + 1] != pos:
                nxt[i + 1] = pos
                changed = True
        if not changed:
            return nsub, passes
        start = list(nxt)


def huffman_lengths(counts):
    """-> code-word length per entry of `counts` of an optimal prefix code (two or more entries). Where counts tie the lengths of single
    symbols may be dealt otherwise by another queue, the total sum(count * length) may not."""
    heap = [(int(c), i, (i,)) for i, c in enumerate(counts)]
    heapq.heapify(heap)
    depth = [0] * len(counts)
    tick = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for i in a[2] + b[2]:
            depth[i] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    return depth


def _equal(n, m):
    return [n // m + (1 if i < n % m else 0) for i in range(m)]


# name -> (counts, order, code-word bits of a fixed-length family or None)
CASES = {}
for _n in (2047, 2048, 2049, 14000, 16384, 17749, 49152):
    CASES["flat8-%d" % _n] = (_equal(_n, 8), "shuffled", 3)
for _n in (8000, 40000):
    CASES["flat32-%d" % _n] = (_equal(_n, 32), "shuffled", 5)
for _n in (4096, 4097, 40000):  # 4096: exactly one subsequence of bits; 4097: seven padding bits, each of them a code word
    CASES["flat2-%d" % _n] = (_equal(_n, 2), "shuffled", 1)
CASES["flat256-65536"] = (_equal(65536, 256), "shuffled", 8)  # 128 whole subsequences
CHAIN17 = [1 << k for k in range(17)]  # no ties, depth 16 > the 12-bit table, n = 131071
DOMINANT = [200000] + [1] * 300
for _o in ("clustered", "shuffled"):
    CASES["chain17-" + _o] = (CHAIN17, _o, None)
    CASES["dominant-" + _o] = (DOMINANT, _o, None)
CASES["one"] = ([5000], "clustered", None)  # a single symbol: a tree of one leaf and no bit stream
FIXTURE_CASES = sorted(CASES)
DTYPE = np.float32

FIB35 = _fib(35)              # 1, 1, 2, 3 ... 9227465: n = F(37) - 1 = 24,157,816, two code words of 34 bits, one symbol of 33
FIB35_N = sum(FIB35)
# (tile, symbol index in the tile, rank by rarity of the symbol placed): a tile of the most frequent symbol's run, whose code word has
# one bit, so the symbol's index in the tile IS the bit offset of its code word in the tile's stage
FIB35_PLACED = ((8000, 31, 0),   # 34 bits at offset 31: 65 bits, the one bit in the third stage word
                (9000, 30, 1),   # 34 bits at offset 30: 64 bits, the two stage words full and no spill
                (10000, 0, 2),   # 33 bits at offset 0: the decoder's window refill with the word aligned
                (11000, 31, 2))  # 33 bits at offset 31: ends with the second stage word


def chain_lengths(counts):
    """the lengths the reference's tree gives rising counts that form a chain (every merged node lighter than the next count but
    one): the rung alone decides, the two rarest share the deepest"""
    m = len(counts)
    return [m - 1] + [m - j for j in range(1, m)]


def stream_bits(name):
    """the stated length in bits of a case's bit stream (before the rounding up to whole bytes)"""
    if name == "fib35":
        return sum(c * l for c, l in zip(FIB35, chain_lengths(FIB35)))
    counts, _, L = CASES[name]
    if L is not None:
        return sum(counts) * L
    if len(counts) == 1:
        return 0
    if counts is CHAIN17:
        return sum(c * l for c, l in zip(counts, chain_lengths(counts)))
    return sum(c * l for c, l in zip(counts, huffman_lengths(counts)))


def regime(name):
    """-> (route, passes or None, exact): what sz3hip_debug_stock_huffman must say after the device stage read the case — passes is
    asserted as equal where `exact`, as an upper bound otherwise"""
    counts, _, L = CASES[name]
    if len(counts) == 1:
        return ROUTE_SINGLE, None, False
    if L is None:
        return ROUTE_DEVICE, MAX_PASSES, False
    _, passes = sync_passes(sum(counts), L)
    return (ROUTE_DEVICE, passes, True) if passes <= MAX_PASSES else (ROUTE_HOST_CAP, None, False)


@functools.lru_cache(maxsize=None)
def crafted(name):
    """-> (array, expected codes) of a case of CASES; cached, read-only"""
    counts, order, _ = CASES[name]
    x, codes = array_from_codes(delta_stream(counts, order), DTYPE)
    x.setflags(write=False)
    codes.setflags(write=False)
    return x, codes


@functools.lru_cache(maxsize=1)
def fib35():
    """-> (array of 24,157,816 f32, expected codes, bit offset of every placed code word in its tile's stage): the rare symbols
    clustered at the start, rarest first, but for the four occurrences of FIB35_PLACED"""
    d = delta_stream(FIB35, "clustered")
    delta = deltas_by_count(FIB35)
    by_rarity = np.argsort(np.asarray(FIB35), kind="stable")
    taken = [delta[by_rarity[r]] for _, _, r in FIB35_PLACED]
    assert list(d[:4]) == taken  # (the clustered order begins with them)
    places = np.array([t * ENC_TILE + k for t, k, _ in FIB35_PLACED], dtype=np.int64)
    out = np.empty(FIB35_N, dtype=np.int64)
    rest = np.ones(FIB35_N, dtype=bool)
    rest[places] = False
    out[places] = taken
    out[rest] = d[4:]
    x, codes = array_from_codes(out, DTYPE)
    x.setflags(write=False)
    codes.setflags(write=False)
    return x, codes


def code_lengths_of(codes, counts, lengths):
    """-> length in bits of every element's code word, given the lengths by entry of `counts` (symbols as deltas_by_count deals them)"""
    table = np.zeros(65536, dtype=np.int64)
    table[deltas_by_count(counts) + RADIUS] = lengths
    return table[codes]


def nopred_config(n):
    from oracle_binding import ALGO_NOPRED, make_config
    return make_config((n,), algo=ALGO_NOPRED, abs_eb=EB)


def unpack(blob):
    """-> (cmprAlgo of the container's trailer, leaves of the tree, elements coded, bytes of the bit stream) of a stock ALGO_NOPRED
    container of f32: [16-byte header][u64 raw length][zstd frame][Config trailer], the raw buffer = quantizer (u8 id, f64 eb, i32
    radius, u64 count + values), tree (i32 offset, be32 nodes, be32, u8, nodes * (2 w + 5) bytes), u64 n, u64 bytes, bits"""
    import ctypes as C
    import sz3_amd
    from oracle_binding import oracle
    b = np.ascontiguousarray(np.frombuffer(bytes(blob), dtype=np.uint8))
    c = sz3_amd.Config(1)
    assert sz3_amd.lib().sz3hip_peek_config(C.byref(c._c), b.ctypes.data, b.size) == 0
    raw_bytes = b.tobytes()
    plen, = struct.unpack_from("<Q", raw_bytes, 8)
    pay = np.frombuffer(raw_bytes[16:16 + plen], dtype=np.uint8)
    rawlen, = struct.unpack_from("<Q", raw_bytes, 16)
    raw = np.empty(rawlen, dtype=np.uint8)
    assert oracle().szo_zstd_decompress(pay.ctypes.data, pay.size, raw.ctypes.data, rawlen) == rawlen
    raw = raw.tobytes()
    uid, eb, radius, n_unpred = struct.unpack_from("<BdiQ", raw, 0)
    assert uid == 2 and eb == EB and radius == RADIUS and n_unpred == 0, (uid, eb, radius, n_unpred)
    at = 21
    nodes, = struct.unpack_from(">I", raw, at + 4)
    w = 1 if nodes <= 256 else (2 if nodes <= 65536 else 4)
    at += 13 + nodes * (2 * w + 5)
    n, bit_bytes = struct.unpack_from("<QQ", raw, at)
    assert nodes == 1 or at + 16 + bit_bytes == rawlen, (at, bit_bytes, rawlen)
    return int(c.cmprAlgo), (nodes + 1) // 2, int(n), int(bit_bytes)
