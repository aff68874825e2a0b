"""CPU tests of the crafted stock streams (tests/crafted_stock.py): every family is held to its stated regime by the reference alone — the
container stays ALGO_NOPRED, decodes to the array bit for bit, and its bit stream has the stated length, which is what makes the
model of the restart-point loop (sync_passes) and the hand-placed code words of fib35 statements about the reference's file and not
about this library. The stored containers (tests/golden/crafted_stock.npz) are held to a fresh run of the reference."""
import os

import numpy as np
import pytest

import crafted_stock as cs
from oracle_binding import ALGO_NOPRED, have_ref, ref_compress, ref_decompress

needs_ref = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libsz3ref.so not built")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crafted_stock.npz")


@pytest.mark.parametrize("L,n,want", [(3, 14000, (11, 11)), (3, 16384, (12, 12)), (3, 17749, (13, 13)), (3, 49152, (36, 36)), (5, 8000, (10, 10)),
                                      (5, 40000, (49, 49)), (8, 65536, (128, 1)), (1, 40000, (10, 1))])
def test_the_model_of_the_restart_point_loop(L, n, want):
    assert cs.sync_passes(n, L) == want


def test_the_regimes_the_families_are_there_for():
    """the cap's two sides, by the model: 12 subsequences of 3-bit codes settle in the last pass the cap allows, 13 do not"""
    assert cs.regime("flat8-14000") == (cs.ROUTE_DEVICE, 11, True)
    assert cs.regime("flat8-16384") == (cs.ROUTE_DEVICE, cs.MAX_PASSES, True)
    assert cs.regime("flat32-8000") == (cs.ROUTE_DEVICE, 10, True)
    for name in ("flat8-17749", "flat8-49152", "flat32-40000"):
        assert cs.regime(name)[0] == cs.ROUTE_HOST_CAP
    for name in ("flat256-65536", "flat2-4096", "flat2-4097", "flat2-40000"):
        assert cs.regime(name) == (cs.ROUTE_DEVICE, 1, True)
    assert cs.regime("one")[0] == cs.ROUTE_SINGLE
    assert cs.stream_bits("flat2-4096") == cs.SUB_BITS and cs.stream_bits("flat256-65536") == 128 * cs.SUB_BITS
    assert cs.stream_bits("flat2-4097") % 8 == 1            # seven padding bits
    assert cs.stream_bits("flat8-16384") == 12 * cs.SUB_BITS
    assert sum(cs.CASES["flat8-2049"][0]) == cs.ENC_TILE + 1  # a last coder tile of one symbol
    # the chains' lengths as the rung gives them are an optimal code's
    for counts in (cs.CHAIN17, cs.FIB35):
        assert sum(c * l for c, l in zip(counts, cs.chain_lengths(counts))) == sum(c * l for c, l in zip(counts, cs.huffman_lengths(counts)))
    assert max(cs.chain_lengths(cs.CHAIN17)) == 16 and max(cs.chain_lengths(cs.FIB35)) == 34 and cs.FIB35_N == 24157816


def _held_to_its_regime(name, x, codes, blob):
    algo, leaves, n, bit_bytes = cs.unpack(blob)
    assert algo == ALGO_NOPRED, "the reference left ALGO_NOPRED (lossless?)"
    assert n == x.size and leaves == np.unique(codes).size
    assert bit_bytes == (cs.stream_bits(name) + 7) // 8, (bit_bytes, cs.stream_bits(name))
    assert np.array_equal(ref_decompress(blob, x.dtype, x.shape).view(np.uint32), x.view(np.uint32)), "the reference does not decode x bit for bit"


@needs_ref
@pytest.mark.parametrize("name", cs.FIXTURE_CASES)
def test_a_family_is_in_its_regime_and_its_stored_container_is_fresh(name):
    x, codes = cs.crafted(name)
    blob = ref_compress(x, cs.nopred_config(x.size))
    _held_to_its_regime(name, x, codes, blob)
    with np.load(FIXTURE) as z:
        assert sorted(z.files) == cs.FIXTURE_CASES
        assert z[name].dtype == np.uint8 and z[name].tobytes() == blob.tobytes(), "tests/golden/crafted_stock.npz is stale: run tests/golden/make_crafted_stock.py"


def test_the_fixture_is_small():
    assert os.path.getsize(FIXTURE) <= 256 * 1024


@needs_ref
def test_fib35_is_in_its_regime_and_its_code_words_sit_where_they_were_placed():
    x, codes = cs.fib35()
    hist = np.bincount(codes, minlength=65536)
    assert x.size == cs.FIB35_N and np.array_equal(hist[cs.deltas_by_count(cs.FIB35) + cs.RADIUS], cs.FIB35)
    blob = ref_compress(x, cs.nopred_config(x.size))
    _held_to_its_regime("fib35", x, codes, blob)
    # every code word's length is known from its rung, so every bit offset is; the stream's length above is the reference's word for it
    lens = cs.code_lengths_of(codes, cs.FIB35, cs.chain_lengths(cs.FIB35))
    assert int(lens.sum()) == cs.stream_bits("fib35")
    want = {(34, 31): "third stage word", (34, 30): "64 bits, no spill", (33, 0): "refill, aligned", (33, 31): "ends with the second word"}
    got = set()
    for tile, k, _ in cs.FIB35_PLACED:
        i = tile * cs.ENC_TILE + k
        got.add((int(lens[i]), int(lens[tile * cs.ENC_TILE:i].sum())))  # (length, bit offset in the tile's stage)
    assert got == set(want)
    # ... and the spill is that one: no other code word of a tile crosses into a third word
    tile_start = np.arange(x.size) // cs.ENC_TILE * cs.ENC_TILE
    before = np.cumsum(lens) - lens
    off = before - before[tile_start]
    assert int(np.count_nonzero(lens + (off & 31) > 64)) == 1
    # the rare symbols are clustered at the start: the first four subsequences hold nothing the 12-bit table decodes
    assert int(lens[before < 4 * cs.SUB_BITS].min()) > 12
