"""One Lorenzo payload of the device API held to the numpy model of the format (tests/szh_ref.py) in full — TEST INFRASTRUCTURE (no tests,
no fixtures): stage-1 codes, both lists, header, book (symbols, Kraft sum, limit, cost; a wide book: tests/widebook_model.py), chunk table,
bit stream, decode. Shared by tests/test_gpu_crafted_codes.py and tests/test_gpu_wide_books.py (streams prescribed symbol by symbol),
tests/checks/sampled_sweep.py (streams of seeded fields) and tests/checks/widebook_sweep.py (streams of drawn histograms)."""
import numpy as np

import sampled_model
import szh_ref
import widebook_model

GROUP = 32  # chunks per offset group of the packers (PACK_GROUP)


def same_codes(got, exp, shape=None):
    """stage 1's codes against the model's; the message names the first element that differs"""
    got, exp = np.asarray(got).reshape(-1), np.asarray(exp).reshape(-1)
    assert got.size == exp.size, "%d codes, %d expected" % (got.size, exp.size)
    neq = np.nonzero(got != exp)[0]
    if neq.size:
        at = int(neq[0])
        where = at if shape is None else tuple(int(v) for v in np.unravel_index(at, shape))
        raise AssertionError("quantisation codes differ from the model's in %d places, first at %s (%d, expected %d)" % (neq.size, where, int(got[at]), int(exp[at])))


def bits_equal(a, b):
    """bit for bit (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view("u%d" % a.itemsize), b.view("u%d" % b.itemsize))


def chunk_picks(h, bits, exp, extra=(), rare=None):
    """the chunks the slow decoder is run on: chunk 0, the last chunk, the densest chunk, the first chunk of offset group 1, the last chunk
    of the last full offset group, one chunk that holds an escape (code 0), the chunk with the most symbols of the rare class (rare: a
    mask over the 65536 codes, two-class books), and `extra`"""
    nc = h["n_chunks"]
    pick = {0, nc - 1, int(np.argmax(bits))}
    if nc > GROUP:
        pick.add(GROUP)
    if nc >= GROUP:
        pick.add((nc // GROUP) * GROUP - 1)
    flat = np.asarray(exp).reshape(-1)
    zeros = np.nonzero(flat == 0)[0]
    if zeros.size:
        pick.add(int(zeros[zeros.size // 2]) // szh_ref.CHUNK)
    if rare is not None and rare.any():
        per = np.zeros(nc * szh_ref.CHUNK, dtype=np.int64)
        per[:flat.size] = rare[flat]
        pick.add(int(np.argmax(per.reshape(nc, szh_ref.CHUNK).sum(axis=1))))
    pick.update(int(c) % nc for c in extra)
    return sorted(pick)


def check_book_and_stream(h, sec, exp, n, st=None, sample=None, extra_chunks=(), full_decode_below=120000, one_class=False, packed=True):
    """the Huffman stage of one payload: the header's book fields, the book, the chunk table of every chunk, bitstream_words, the slow
    decoder on chunk_picks. h, sec: szh_ref.parse's; exp: the codes the stream holds, in the packer's order; st: the call's stats (None:
    a stream that is not a Lorenzo payload's — no sampled book, no rule about the format's version); sample: see check_payload;
    one_class: a wide book must be the one-class construction (widebook_model.check_wide_book); packed=False: book and bitstream_words
    only. A stream whose book the wide construction builds (widebook_model.path) is held to widebook_model.check_wide_book, every other
    to a Kraft sum of 1 and szh_ref.assert_book_optimal. -> figures"""
    exp = np.asarray(exp).reshape(-1)
    lens = sec["lens"].astype(np.int64)
    present = np.unique(exp)
    have = set((h["sym_min"] + np.nonzero(lens)[0]).tolist())
    freq = np.bincount(exp, minlength=65536)[h["sym_min"]:h["sym_min"] + h["sym_count"]].astype(np.int64)
    kraft_units = sum(1 << (szh_ref.MAX_LEN - int(l)) for l in lens[lens > 0])
    assert h["max_len"] == lens.max() and (st is None or h["max_len"] == st["max_code_len"])
    book = wide = rare = None
    if h["esc_sym"]:
        # the sampled book: a code word for every byte value, whatever the sample met; code 0 (a listed delta) rides the escape symbol
        assert st["narrow_codes"] == 1 and n >= 1 << 22
        assert h["esc_sym"] == h["radius"] + 128 and h["sym_min"] == h["radius"] - 127 and h["sym_count"] == 256 and h["version"] == 5
        assert set(present[present > 0].tolist()) <= have and h["esc_sym"] in have
        freq[255] += int(np.count_nonzero(exp == 0))
        assert freq.sum() == n
        assert kraft_units <= 1 << szh_ref.MAX_LEN and lens.max() <= szh_ref.MAX_LEN
        limit = szh_ref.MAX_LEN
        bfreq = freq
        if sample is not None:
            book = sampled_model.check_book(lens, sample)
    else:
        assert sample is None, "the stream must have a sampled book and has none"
        assert st is None or h["version"] == 4
        syms, filled = szh_ref.book_symbols(present)
        assert have == syms, "the book's symbols are not the stream's (+ margins)"
        limit = szh_ref.SHORT_LEN if len(syms) <= szh_ref.SHORT_SYMS else szh_ref.MAX_LEN
        is_wide = widebook_model.path(freq) != widebook_model.SMALL
        if is_wide:  # (no margins there: the book's histogram is the stream's)
            assert not filled and h["sym_min"] == present.min() and h["sym_count"] == present.max() - present.min() + 1 and freq.sum() == n
            wide = widebook_model.check_wide_book(lens, freq, h["sym_min"], one_class=one_class)
            if wide["two_class"]:
                rare = np.zeros(65536, dtype=bool)
                rare[h["sym_min"]:h["sym_min"] + h["sym_count"]] = (freq > 0) & (freq <= wide["rule"]["rare_max"])
            bfreq = freq
        else:
            assert kraft_units == 1 << szh_ref.MAX_LEN, "Kraft sum %d / 2^24" % kraft_units
            assert lens.max() <= limit
            bfreq, bmin, blimit = szh_ref.book_histogram(np.bincount(exp, minlength=65536)[present.min():present.max() + 1], int(present.min()))
            assert blimit == limit and freq.sum() == n
            if filled:
                assert h["sym_min"] == bmin == min(syms) and h["sym_count"] == len(syms) == len(bfreq)
                assert np.array_equal(np.maximum(freq, 1), bfreq)
            else:
                assert h["sym_min"] == bmin and h["sym_count"] == len(bfreq) and np.array_equal(freq, bfreq)
    # the book's cost: never below the length-limited optimum; the project's rule against the unlimited code; the kernel's documented loss
    pm = szh_ref.package_merge_lengths(bfreq, limit)
    pm_cost, gpu_cost = int((bfreq * pm).sum()), int((bfreq * lens).sum())
    unlimited, height = szh_ref.huffman_cost(bfreq)
    bits, chunkwords, subbits = szh_ref.chunk_table(exp, lens, h["sym_min"], h["esc_sym"])
    fig = dict(narrow=int(st["narrow_codes"]) if st is not None else 0, symbols=len(bfreq), limit=limit, max_len=int(lens.max()), height=height,
               over_pm=(gpu_cost - pm_cost) / n, over_unlimited=(gpu_cost - unlimited) / n, densest=float(bits.max()) / (szh_ref.CHUNK * limit), book=book, wide=wide)
    if not h["esc_sym"] and wide is None:
        assert pm_cost <= gpu_cost, "the book costs less than the length-limited optimum: not a code of that limit"
        szh_ref.assert_book_optimal(bfreq, lens, limit)
        if len(bfreq) <= szh_ref.SHORT_SYMS:
            assert (gpu_cost - unlimited) / n < 0.01, "16-bit limit: %.5f bit/symbol over the unlimited code" % ((gpu_cost - unlimited) / n)
    # the packed stream: the chunk table of the whole payload from the payload's own lengths, the slow decoder on the picked chunks
    assert h["n_chunks"] == len(bits) and h["bitstream_words"] == int(chunkwords.sum())
    if not packed:
        return fig
    assert np.array_equal(sec["chunkwords"], chunkwords), "chunkwords differ from the lengths' sums"
    assert np.array_equal(sec["subbits"], subbits), "restart offsets differ from the lengths' sums"
    if n <= full_decode_below:
        assert np.array_equal(szh_ref.huffman_decode(h, sec), exp), "the bit stream does not decode to the model's codes"
    else:
        pick = chunk_picks(h, bits, exp, extra_chunks, rare)
        got = szh_ref.huffman_decode(h, sec, chunks=pick)
        for c in pick:
            sl = slice(c * szh_ref.CHUNK, (c + 1) * szh_ref.CHUNK)
            assert np.array_equal(got[sl], exp[sl]), "chunk %d does not decode to the model's codes" % c
    return fig


def check_payload(x, eb, exp, dout_idx, dout_val, vout_idx, blob, codes, st, dec, sample=None, extra_chunks=(), full_decode_below=120000, one_class=False):
    """everything asked of one payload. x: the array; exp: the codes stage 1 must emit (flat); dout_idx / dout_val: the listed deltas'
    places (rising) and values; vout_idx: the places of the listed values (rising); codes, st, dec: debug_codes, stats and the device's
    decode of the payload; sample: the sample's 256 counts where the stream must have a sampled book (None: the exact histogram's book,
    or a sampled book held to the header rules and to a valid prefix code only); one_class: check_book_and_stream's. -> (header, figures)"""
    n = x.size
    exp = np.asarray(exp).reshape(-1)
    same_codes(codes, exp, x.shape)
    h, o, sec = szh_ref.parse(blob)
    assert h["magic"] == szh_ref.MAGIC and h["n"] == n and h["payload_bytes"] == len(blob) == st["payload_bytes"]
    # both lists: the model's indices, in index order, and the model's values
    assert h["n_vout"] == len(vout_idx) == st["n_value_outliers"], "listed values: %d, the model lists %d" % (h["n_vout"], len(vout_idx))
    assert h["n_dout"] == len(dout_idx) == st["n_delta_outliers"], "listed deltas: %d, the model lists %d" % (h["n_dout"], len(dout_idx))
    assert np.array_equal(sec["dout_idx"].astype(np.int64), dout_idx), "the listed deltas' places differ from the model's (or are out of order)"
    assert np.array_equal(sec["dout_val"].astype(np.int64), np.asarray(dout_val, dtype=np.int64)), "the listed deltas' values differ from the model's"
    assert np.array_equal(sec["vout_idx"].astype(np.int64), vout_idx), "the listed values' places differ from the model's (or are out of order)"
    assert bits_equal(sec["vout_val"], x.reshape(-1)[np.asarray(vout_idx, dtype=np.int64)]), "the listed values are not the array's"
    fig = check_book_and_stream(h, sec, exp, n, st, sample, extra_chunks, full_decode_below, one_class)
    # the decode: the model's array bit for bit, within the bound at every finite point, NaN where the input has it
    model = szh_ref.reconstruct(h, sec, exp).reshape(x.shape)
    assert bits_equal(dec, model), "the decoder's array differs from the model's"
    fin = np.isfinite(x)
    if fin.any():
        err = float(np.max(np.abs(dec[fin].astype(np.float64) - x[fin].astype(np.float64))))
        assert err <= eb, "max error %g beyond the bound %g" % (err, eb)
    assert np.array_equal(np.isnan(dec), np.isnan(x)), "NaN is not where the input has it"
    return h, fig
