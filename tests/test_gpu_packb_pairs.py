"""GPU tests (-m gpu) of k_pack_b's pair table as it is addressed since round 20: entry (t0 & 127) + PB_PAIR_STRIDE * (t1 & 127), one
dot product per pair, rows padded to an odd stride. The code streams are prescribed symbol by symbol (tests/crafted_codes.py), 2^22
elements each — the smallest array that reaches k_pack_b with the sampled book (4096 chunks):
  every cell   deltas uniform over the window's 128 bytes: each of the 16 384 ordered pairs stands at an even place of the stream, so
               every cell of the table is read, and every chunk takes the fast tier;
  aliases      the same stream with the bytes 63 and 192 put in, which the 7-bit mask turns into the window bytes 191 and 64: their
               chunks must leave the fast tier, not take the alias's code word;
  no entry     fib17 x 56, shuffled: pairs longer than 27 bits and values the sample never met, beside fast chunks.
Under the exact book k_pack_b is held to k_pack's bytes (same book, same chunk table); under the sampled book, which is k_pack_b's
alone, to the prescribed array on decode, to itself across calls and contexts, and both forms of the kernel (the offset scan inside
the launch, k_pack_b<true>, or in a launch of its own, k_pack_b<false>) to each other."""
import functools

import numpy as np
import pytest

import sz3_amd
import crafted_codes as cc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

Dbg = sz3_amd.Dbg
SCAN_LAUNCH = sz3_amd.Dbg2.PACK_SCAN_LAUNCH
EB = cc.EB
SHAPE = (2048, 2048)              # 2^22 elements, rows of whole 256-element segments
CHUNK = 1024                      # symbols of a chunk
BYTE0 = 127                       # a one-byte code is the delta + 127 (the sampled book's header: sym_min = radius - 127)
WINDOW = (64, 192)                # the pair table's bytes


def _conf(shape):
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
    c.regression = 0
    c.errorBoundMode = sz3_amd.EB_ABS
    c.absErrorBound = EB
    return c


@functools.lru_cache(maxsize=1)
def _window_deltas():
    d = np.random.default_rng(20).integers(WINDOW[0] - BYTE0, WINDOW[1] - BYTE0, SHAPE[0] * SHAPE[1], dtype=np.int64)  # -63 .. +64
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=1)
def _alias_deltas():
    """the window stream with 150 deltas of -64 (byte 63) and 150 of +65 (byte 192): a hundred at even places, a hundred at odd places,
    a hundred on both sides of fifty chunk borders; -> (deltas, their places)"""
    d = _window_deltas().copy()
    rng = np.random.default_rng(21)
    chunks = 2 * rng.choice(d.size // CHUNK // 2 - 1, 250, replace=False)  # one chunk per place (even ones: a border's second chunk is odd), the others stay in the fast tier
    even = chunks[:100] * CHUNK + 2 * rng.integers(1, CHUNK // 2 - 1, 100)
    odd = chunks[100:200] * CHUNK + 2 * rng.integers(1, CHUNK // 2 - 1, 100) + 1
    border = (chunks[200:] + 1) * CHUNK
    places = np.concatenate([even, odd, border - 1, border])
    d[places] = np.where(np.arange(places.size) % 2 == 0, WINDOW[0] - 1 - BYTE0, WINDOW[1] - BYTE0)
    d.setflags(write=False)
    return d, places


@functools.lru_cache(maxsize=3)
def _array(which):
    if which == "noentry":
        x, codes = cc.crafted(cc.SAMPLED_FAMILY, "shuffled", np.float32, cc.SAMPLED_SHAPE)
        return x, codes
    d = _window_deltas() if which == "window" else _alias_deltas()[0]
    x, codes = cc.array_from_deltas(d, np.float32, SHAPE)
    x.setflags(write=False)
    codes.setflags(write=False)
    return x, codes


def _calls(x, flags=0, flags2=0, calls=3):
    """a fresh context, `calls` compressions of x (the first call of a context waits for the probe: the one-launch stage 1 and with it
    k_pack_b from the second call on) -> (payloads, the encoder's launches of every call, stage 1's codes, stats, the last payload decoded)"""
    dev = torch.device("cuda:0")
    t = torch.from_numpy(x.copy()).to(dev)  # (the cached array is read-only)
    dc = sz3_amd.DeviceCompressor(x.size, x.dtype)
    cap = dc.payload_bound(x.size, worst_case=True)
    pl = torch.empty(cap, dtype=torch.uint8, device=dev)
    outs, launches = [], []
    with sz3_amd.debug_flags(int(flags)), sz3_amd.debug_flags2(int(flags2)):
        for _ in range(calls):
            size = dc.compress(_conf(x.shape), t.data_ptr(), pl.data_ptr(), cap, 0)
            launches.append(sz3_amd.last_encode_launches())
            outs.append(pl[:size].cpu().numpy().tobytes())
        codes = dc.debug_codes(x.size)
    st = dc.stats()
    dec = torch.empty_like(t)
    dc.decompress(pl.data_ptr(), size, dec.data_ptr(), 0)
    torch.cuda.synchronize()
    return outs, launches, codes, st, dec.cpu().numpy()


def _sampled(blob):
    import szh_ref
    h, _, _ = szh_ref.parse(np.frombuffer(blob, dtype=np.uint8))
    return h["esc_sym"] != 0  # (the header's escape symbol: sampled books only)


def _against_k_pack(x, prescribed):
    """the exact book: k_pack_b's payload is k_pack's, call by call, and decodes within the bound"""
    new, _, codes, st, dec = _calls(x, Dbg.CB_NO_SAMPLED)
    old, _, _, _, _ = _calls(x, Dbg.CB_NO_SAMPLED | Dbg.PACK_OLD)
    assert st["narrow_codes"], "two-byte codes: not this packer's case"
    assert np.array_equal(codes, prescribed), "stage 1 did not emit the prescribed stream"
    assert not _sampled(new[2])
    for k in range(3):
        assert new[k] == old[k], "call %d: k_pack_b and k_pack disagree" % k
    assert np.max(np.abs(dec.astype(np.float64) - x.astype(np.float64))) <= EB
    return new


def _sampled_book(x, prescribed, flags2=0, launches=2):
    """the sampled book: one payload in all three calls, the prescribed array on decode, the expected launches; -> the payload"""
    outs, l, codes, st, dec = _calls(x, 0, flags2)
    assert st["narrow_codes"] and _sampled(outs[2]), "the call did not code with a sampled book"
    assert np.array_equal(codes, prescribed), "stage 1 did not emit the prescribed stream"
    assert outs[0] == outs[1] == outs[2], "a repeated call writes another payload"
    assert np.array_equal(dec, x), "the stream does not decode to the prescribed array"
    assert l[1:] == [launches, launches], l  # the segment pass and the packer (+ the offset scan's own launch)
    return outs[2]


def test_window_stream_reads_every_cell():
    """the reference stream alone: every ordered pair of window bytes at an even place, the prefix sums inside array_from_deltas' bound"""
    d = _window_deltas()
    b = d + BYTE0
    assert WINDOW[0] <= b.min() and b.max() < WINDOW[1]
    pair = (b[0::2] - WINDOW[0]) * 128 + (b[1::2] - WINDOW[0])
    seen = np.bincount(pair, minlength=128 * 128)
    assert seen.size == 128 * 128 and seen.min() >= 1, "a pair of the table is never looked up"
    q = np.cumsum(np.cumsum(d.reshape(SHAPE), axis=0), axis=1)
    assert int(np.abs(q).max()) < 1 << 22
    da, places = _alias_deltas()
    ba = da + BYTE0
    out = (ba < WINDOW[0]) | (ba >= WINDOW[1])
    assert np.array_equal(np.sort(np.nonzero(out)[0]), np.sort(places)) and places.size == 300
    assert set(ba[out].tolist()) == {WINDOW[0] - 1, WINDOW[1]}
    assert np.count_nonzero(places % 2 == 0) == 150 and np.count_nonzero(places % CHUNK == 0) == 50 and np.count_nonzero(places % CHUNK == CHUNK - 1) == 50
    assert np.unique(places // CHUNK).size == 300  # (no two in one chunk: 3796 chunks of the 4096 hold window bytes only)


def test_every_cell_exact_book():
    x, prescribed = _array("window")
    _against_k_pack(x, prescribed)


def test_every_cell_sampled_book_both_forms():
    x, prescribed = _array("window")
    in_launch = _sampled_book(x, prescribed)                        # k_pack_b<true>
    own_launch = _sampled_book(x, prescribed, SCAN_LAUNCH, 3)       # k_pack_b<false>
    assert in_launch == own_launch, "the two forms of the kernel write different bytes"


def test_aliases_leave_the_fast_tier():
    x, prescribed = _array("alias")
    _against_k_pack(x, prescribed)
    _sampled_book(x, prescribed)


def test_pairs_without_an_entry():
    x, prescribed = _array("noentry")
    a = _sampled_book(x, prescribed)
    b = _sampled_book(x, prescribed)  # another context
    assert a == b, "two contexts write different payloads"
