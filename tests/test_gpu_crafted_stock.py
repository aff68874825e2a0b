"""GPU tests (-m gpu): the crafted stock streams of tests/crafted_stock.py shown to the device's stock Huffman stage (sz3hip_stock.hip:
k_stock_huff_sync, k_stock_huff_write, stock_decode_one, k_stock_enc_bits, k_stock_enc_pack) and to stock_huff_run behind it. The
containers are the reference's own files (tests/golden/crafted_stock.npz, kept fresh by tests/test_crafted_stock_cpu.py, which also
proved that the reference decodes each of them to the array it was made from), so the read direction needs no reference here. What the
decoder did — restart-point passes, device or host — is read from sz3hip_debug_stock_huffman and held to the model of the pass loop
(crafted_stock.sync_passes): fixed-length codes of 3 and 5 bits take one pass per subsequence, up to the cap and beyond it."""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sz3_amd  # noqa: E402
import crafted_stock as cs  # noqa: E402
from oracle_binding import ALGO_LORENZO_REG, have_ref, make_config, ref_compress, ref_decompress  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crafted_stock.npz")
ROUTES = {cs.ROUTE_DEVICE: "device", cs.ROUTE_HOST_SWITCH: "host by the switch", cs.ROUTE_HOST_CAP: "host after the cap", cs.ROUTE_SINGLE: "single symbol"}


@pytest.fixture(scope="module")
def containers():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _read(blob, x, monkeypatch, host):
    monkeypatch.setenv("SZ3HIP_STOCK_HOST_HUFFMAN", "1" if host else "0")
    got, conf = sz3_amd.decompress(blob, x.dtype, x.shape)
    assert conf.cmprAlgo == sz3_amd.ALGO_NOPRED
    return got, sz3_amd.debug_stock_huffman()


def _write(x, monkeypatch, host):
    monkeypatch.setenv("SZ3HIP_STOCK_HOST_HUFFMAN", "1" if host else "0")
    conf = sz3_amd.Config(*x.shape)
    conf.cmprAlgo = sz3_amd.ALGO_NOPRED
    conf.absErrorBound = cs.EB
    conf.regression = 0  # (make_config's: the Config trailer holds the flags whatever the algorithm)
    L = sz3_amd.lib()
    L.sz3hip_set_stock_format(1)
    try:
        blob, _ = sz3_amd.compress(x, conf)
    finally:
        L.sz3hip_set_stock_format(0)
    return blob


def _assert_regime(name, passes, route):
    want_route, want_passes, exact = cs.regime(name)
    print("%s: route %d (%s), %d passes on the device; the model: route %d, %s passes" % (name, route, ROUTES.get(route), passes, want_route, want_passes))
    assert route == want_route, "%s went %s, the model says %s" % (name, ROUTES.get(route), ROUTES[want_route])
    if want_route == cs.ROUTE_DEVICE:
        assert (passes == want_passes) if exact else (1 <= passes <= want_passes), (passes, want_passes)
    elif want_route == cs.ROUTE_HOST_CAP:
        assert passes == cs.MAX_PASSES  # every launch the cap allows was made before the host took over
    else:
        assert passes == 0


@pytest.mark.parametrize("name", cs.FIXTURE_CASES)
def test_the_reference_s_container_is_read_bit_for_bit(name, containers, monkeypatch):
    """device stage and host stage read the reference's file to the array it was made from, and the device stage went the way the
    family is there for"""
    x, _ = cs.crafted(name)
    got, (passes, route) = _read(containers[name], x, monkeypatch, host=False)
    assert _same_bits(got, x), "the device stage decodes other values than the reference"
    _assert_regime(name, passes, route)
    got_host, (passes_host, route_host) = _read(containers[name], x, monkeypatch, host=True)
    assert _same_bits(got_host, x) and _same_bits(got_host, got)
    assert (passes_host, route_host) == ((0, cs.ROUTE_SINGLE) if route == cs.ROUTE_SINGLE else (0, cs.ROUTE_HOST_SWITCH))


@pytest.mark.parametrize("fallback,after", [("flat8-17749", "flat8-16384"), ("flat32-40000", "chain17-clustered"), ("flat8-49152", "flat2-4097")])
def test_the_fallback_leaves_the_scratch_usable(fallback, after, containers, monkeypatch):
    """twelve launches wrote restart points and counts of a stream that did not settle into the slot's scratch before the host walked it:
    the next device decode of the same process, of a stream with fewer subsequences, is right and goes its own way"""
    x, _ = cs.crafted(fallback)
    got, (_, route) = _read(containers[fallback], x, monkeypatch, host=False)
    assert _same_bits(got, x) and route == cs.ROUTE_HOST_CAP
    y, _ = cs.crafted(after)
    got, (passes, route) = _read(containers[after], y, monkeypatch, host=False)
    assert _same_bits(got, y)
    _assert_regime(after, passes, route)


@pytest.mark.parametrize("name", cs.FIXTURE_CASES)
def test_the_written_container_is_the_reference_s_file(name, containers, monkeypatch):
    """sz3hip_set_stock_format(1) + ALGO_NOPRED: the same codes, the reference's tree, one zstd frame (every buffer here is below 1 MB) —
    byte for byte the stored file, from the device coder and from the host coder, and read back to x"""
    x, _ = cs.crafted(name)
    want = containers[name].tobytes()
    for host in (False, True):
        blob = _write(x, monkeypatch, host)
        assert blob.tobytes() == want, "%s coder: %d bytes written, the reference's file has %d" % ("host" if host else "device", len(blob), len(want))
    back, _ = _read(blob, x, monkeypatch, host=False)
    assert _same_bits(back, x)


def test_fib35_code_words_beyond_32_bits_both_ways(monkeypatch):
    """35 Fibonacci counts, 24,157,816 elements (about 97 MB of f32; no smaller array has a code word of 34 bits): stock_decode_one's window
    refill (code words of 33 bits and more) and k_stock_enc_pack's third stage word (34 bits from bit 31 of a word), which nothing
    else in the suite reaches. tests/test_crafted_stock_cpu.py shows where the code words sit."""
    if not have_ref():
        pytest.skip("oracle/_ref/libsz3ref.so not built")
    t0 = time.perf_counter()
    x, _ = cs.fib35()
    rblob = ref_compress(x, cs.nopred_config(x.size))
    t1 = time.perf_counter()
    got, (passes, route) = _read(rblob, x, monkeypatch, host=False)
    t2 = time.perf_counter()
    assert _same_bits(got, x), "the device stage decodes other values than the reference"
    assert route == cs.ROUTE_DEVICE and 1 <= passes <= cs.MAX_PASSES, (passes, route)
    del got
    monkeypatch.setenv("SZ3HIP_STOCK_ONE_FRAME", "1")  # (7.9 MB of buffer: several frames otherwise)
    for host in (False, True):
        blob = _write(x, monkeypatch, host)
        assert blob.tobytes() == rblob.tobytes(), "%s coder: not the reference's file (%d bytes, %d)" % ("host" if host else "device", len(blob), len(rblob))
    t3 = time.perf_counter()
    assert _same_bits(ref_decompress(blob, x.dtype, x.shape), x)
    print("fib35: array and reference %.2f s, device read %.2f s (%d passes), two writes %.2f s, reference read %.2f s"
          % (t1 - t0, t2 - t1, passes, t3 - t2, time.perf_counter() - t3))


def test_the_stage_is_shared_a_lorenzo_stream_of_the_same_codes(monkeypatch):
    """the flat8 stream of 17749 codes through another reader: as first differences of a 1-D array (crafted_codes.array_from_deltas) the
    reference's ALGO_LORENZO_REG, Lorenzo only, codes it to the same 3-bit stream of 13 subsequences (6656 bytes, read on the CPU) —
    the reader's Huffman stage is the same stock_huff_run and leaves for the host after the cap"""
    if not have_ref():
        pytest.skip("oracle/_ref/libsz3ref.so not built")
    from crafted_codes import array_from_deltas, delta_stream
    x, _ = array_from_deltas(delta_stream(cs.CASES["flat8-17749"][0], "shuffled"), np.float32)
    rblob = ref_compress(x, make_config(x.shape, algo=ALGO_LORENZO_REG, abs_eb=cs.EB, lorenzo=True, regression=False))
    assert cs.unpack(rblob)[1:] == (8, 17749, 6656)
    monkeypatch.setenv("SZ3HIP_STOCK_HOST_HUFFMAN", "0")
    got, conf = sz3_amd.decompress(rblob, x.dtype, x.shape)
    assert conf.cmprAlgo == sz3_amd.ALGO_LORENZO_REG
    assert _same_bits(got, ref_decompress(rblob, x.dtype, x.shape))
    passes, route = sz3_amd.debug_stock_huffman()
    assert route == cs.ROUTE_HOST_CAP or passes > 3, (passes, route)
