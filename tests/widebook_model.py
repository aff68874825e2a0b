"""numpy rules for what the wide code book decides — TEST INFRASTRUCTURE (no tests, no fixtures).

A restatement of codebook_wide (sz3_amd/csrc/sz3hip_kernels.hip, "1b. two-class mode" through step 6) over the histogram of the codes a
stream emits — all bins counted, code 0 included where it occurs. Everything the device decides there is a function of that histogram:
  path(freq)            which construction builds the book                                   (szk_cb_part, the `cls` test of codebook_wide)
  limit(m)              the longest code word a book of m symbols may have                   (CB_SHORT_SYMS, SZH_MAX_LEN)
  class_rule(freq)      the two-class rule: tier, octave, rare class, the class's weight     (step 1b)
  class_weights(...)    the weights the two-class Huffman construction runs on
  model_lens(freq)      a length table that keeps every rule (package-merge: an optimal code of the limit)
  check_wide_book(...)  a payload's length table against all of it
tests/test_widebook_model_cpu.py holds these rules to a second, plainly written form and the constants to the sources' #defines."""
import numpy as np

import szh_ref

# the constants, each once, with its source line
SZK_CB_SMALL_SYMS = 256     # sz3hip_kernels.h:155   alphabets up to this size: the small book
SZK_CB_PART0_SYMS = 640     # sz3hip_kernels.h:160   ... and up to this size where the occupied span is at most
SZK_CB_PART0_RANGE = 4096   # sz3hip_kernels.h:161   ... this many bins
CB_SHORT_SYMS = 512         # sz3hip_kernels.hip     alphabets up to this size are limited to 16-bit code words
SHORT_LEN = 16
SZH_MAX_LEN = 24            # sz3hip_format.h:43
CB_CLASS_MIN = 4096         # sz3hip_kernels.hip     the two-class form is considered beyond this many symbols
CB_CLASS_KEEP = 3072        # sz3hip_kernels.hip     tier 1 keeps at most this many symbols one by one
CB_CLASS_KEEP2 = 12288      # sz3hip_kernels.hip     tier 2
CLASS_SHARE = 64            # codebook_wide: `mass * 64ull <= total` — the rare class may hold 1/64 of the occurrences (estimated)
ROOM_SLACK = 3              # codebook_wide: `room = L > rare_bits + 3 ? L - rare_bits - 3 : 1`
OCTAVES = 48                # counts per octave: floor(log2(count)), capped at 47
CB_LDS_KEYS = 131072 // 8   # CB_POOL_BYTES / 8: up to this many keys the merge's queues and the depth arrays live in LDS

SMALL, WIDE1, WIDE2 = "small", "wide1", "wide2"


def _counts(freq):
    freq = np.asarray(freq, dtype=np.int64)
    nz = np.nonzero(freq)[0]
    return freq, nz


def limit(m):
    """the longest code word of a book of m symbols"""
    return SHORT_LEN if m <= CB_SHORT_SYMS else SZH_MAX_LEN


def path(freq):
    """-> "small" (cb_small), "wide1" (codebook_wide<false>) or "wide2" (codebook_wide<true>: the two-class form is CONSIDERED; class_rule
    says whether a tier is taken)"""
    freq, nz = _counts(freq)
    m = len(nz)
    span = int(nz[-1] - nz[0]) + 1 if m else 0
    if m <= SZK_CB_SMALL_SYMS or (m <= SZK_CB_PART0_SYMS and span <= SZK_CB_PART0_RANGE):
        return SMALL
    return WIDE2 if m > CB_CLASS_MIN else WIDE1


def octaves(freq):
    """-> oct[j], j < 48: the number of symbols whose count has floor(log2(count)) == j (47: that or more)"""
    freq, nz = _counts(freq)
    c = freq[nz]
    j = np.zeros(len(c), dtype=np.int64)
    for b in range(1, 64):
        j += (c >> b) > 0
    return np.bincount(np.minimum(j, OCTAVES - 1), minlength=OCTAVES).astype(np.int64)


def class_rule(freq, octave_shift=0):
    """-> None (one class: not considered, or both tiers rejected) or dict(keep, k, rare_max, n_rare, n_freq, rare_bits, w_rare,
    floor_engaged, total, rare_true). octave_shift: added to the octave a taken tier stops at (tests of the tests)"""
    freq, nz = _counts(freq)
    m = len(nz)
    if path(freq) != WIDE2:
        return None
    total = int(freq.sum())
    oct_ = octaves(freq)
    L = limit(m)
    for keep in (CB_CLASS_KEEP, CB_CLASS_KEEP2):
        if m <= keep + keep // 4:
            continue  # (nothing to gain)
        above, k = 0, OCTAVES - 1
        while k >= 0 and above + int(oct_[k]) <= keep:
            above += int(oct_[k])
            k -= 1
        mass = sum(int(oct_[j]) * (3 << j) // 2 for j in range(k + 1))
        if not (k >= 0 and mass * CLASS_SHARE <= total):
            continue
        k += octave_shift
        rare_max = (2 << k) - 1
        c = freq[nz]
        n_rare = int(np.count_nonzero(c <= rare_max))
        n_freq = m - n_rare
        rare_bits = 0 if n_rare <= 1 else int(n_rare - 1).bit_length()
        room = L - rare_bits - ROOM_SLACK if L > rare_bits + ROOM_SLACK else 1
        fsum = int(c[c > rare_max].sum())
        w_true, w_min = total - fsum, (total >> room) + 1
        return dict(keep=keep, k=k, rare_max=rare_max, n_rare=n_rare, n_freq=n_freq, rare_bits=rare_bits, w_rare=max(w_true, w_min),
                    floor_engaged=w_true < w_min, total=total, rare_true=w_true)
    return None


def class_weights(freq, rule, floor=True):
    """-> (weights: the frequent symbols' counts in symbol order, then the class's; frequent mask over freq; rare mask over freq).
    floor=False: the class's true weight (tests of the tests)"""
    freq, _ = _counts(freq)
    frequent = freq > rule["rare_max"]
    rare = (freq > 0) & ~frequent
    return np.concatenate([freq[frequent], [rule["w_rare"] if floor else rule["rare_true"]]]), frequent, rare


def model_lens(freq, one_class=False, rule="model", floor=True):
    """-> a length table over `freq` that keeps every rule: package-merge over the counts (one class) or over the frequent counts and
    the class's weight, the rare symbols at the class's length + rare_bits. Raises ValueError where the two-class form would fall back
    (a rare symbol's code word longer than the limit). rule: another verdict than class_rule's (tests of the tests)"""
    freq, nz = _counts(freq)
    rule = class_rule(freq) if isinstance(rule, str) else rule
    L = limit(len(nz))
    if one_class or rule is None:
        return szh_ref.package_merge_lengths(freq, L)
    w, frequent, rare = class_weights(freq, rule, floor)
    lv = szh_ref.package_merge_lengths(w, L)
    lens = np.zeros(len(freq), dtype=np.int64)
    lens[frequent] = lv[:-1]
    lens[rare] = lv[-1] + rule["rare_bits"]
    if lv[-1] + rule["rare_bits"] > L:
        raise ValueError("the class's code word of %d bits + %d index bits exceed %d" % (lv[-1], rule["rare_bits"], L))
    return lens


def _units(lens):
    lens = np.asarray(lens, dtype=np.int64)
    return int(np.sum(np.int64(1) << (SZH_MAX_LEN - lens[lens > 0])))


def _held_to_optimum(what, w, lv, L, fig):
    """sum(w * len) against the Huffman cost of w: equal where that tree respects the limit; else no less than package-merge's and
    within the project's 0.2 % of the unlimited code (szh_ref.assert_book_optimal)"""
    cost = int((np.asarray(w, dtype=np.int64) * np.asarray(lv, dtype=np.int64)).sum())
    huff, height = szh_ref.huffman_cost(w)
    fig.update(height=height, limit_binds=height > L, cost=cost, huffman_cost=huff, pm_cost=huff)
    if height <= L:
        assert cost == huff, "optimum: %s costs %d bits, the Huffman code %d (height %d <= %d)" % (what, cost, huff, height, L)
    else:
        pm = szh_ref.package_merge_lengths(w, L)
        fig["pm_cost"] = int((np.asarray(w, dtype=np.int64) * pm).sum())
        assert cost >= fig["pm_cost"], "limit: %s costs less than the %d-bit optimum: not a code of that limit" % (what, L)
        assert cost <= huff * 1.002, "0.2 %% rule: %s costs %d bits, the unlimited code %d (+%.3f %%; package-merge +%.3f %%)" % (
            what, cost, huff, 100.0 * (cost - huff) / huff, 100.0 * (fig["pm_cost"] - huff) / huff)


def check_wide_book(lens, freq, sym_min=0, one_class=False):
    """a payload's length table (entry i: symbol sym_min + i) against the histogram `freq` of the same bins.
    one_class: the book must be the one-class construction whatever class_rule says (CB_ONE_CLASS, or the fallback of a two-class book
    whose rare code words would exceed the limit). -> dict of figures; raises AssertionError whose message names the rule broken."""
    lens = np.asarray(lens).astype(np.int64)
    freq, nz = _counts(freq)
    assert lens.shape == freq.shape
    m = len(nz)
    L = limit(m)
    total = int(freq.sum())
    rule = None if one_class else class_rule(freq)
    assert np.array_equal(lens > 0, freq > 0), "symbols: code words for %d symbols, %d occur (first difference at symbol %d)" % (
        int(np.count_nonzero(lens)), m, sym_min + int(np.nonzero((lens > 0) != (freq > 0))[0][0]))
    assert int(lens.max()) <= L, "limit: a code word of %d bits in a book of %d symbols (limit %d)" % (int(lens.max()), m, L)
    units = _units(lens)
    fig = dict(symbols=m, limit=L, path=path(freq), two_class=rule is not None, max_len=int(lens.max()), kraft_units=units, rule=rule,
               mk=m if rule is None else rule["n_freq"] + 1, len_cls=0)
    book_cost = int((freq * lens).sum())
    one_cost, one_height = szh_ref.huffman_cost(freq)
    fig.update(natural_height=one_height, over_one_class=(book_cost - one_cost) / float(total))
    if rule is None:
        assert units == 1 << SZH_MAX_LEN, "Kraft: the one-class book's sum is %d / 2^24, not 1" % units
        _held_to_optimum("the one-class book", freq, lens, L, fig)
        if m <= CB_SHORT_SYMS:
            assert (book_cost - one_cost) / float(total) < 0.01, "16-bit limit: %.5f bit/symbol over the unlimited code" % ((book_cost - one_cost) / float(total))
        return fig
    w, frequent, rare = class_weights(freq, rule)
    lr = lens[rare]
    assert np.all(lr == lr[0]), "rare class: the %d rare symbols' code words have lengths %s, not one" % (rule["n_rare"], sorted(set(lr.tolist())))
    len_rare = int(lr[0])
    len_cls = len_rare - rule["rare_bits"]
    fig["len_cls"] = len_cls
    assert len_cls >= 1 and len_rare <= L, "rare class: %d bits are not a class code word of 1 .. %d bits + %d index bits" % (len_rare, L - rule["rare_bits"], rule["rare_bits"])
    lv = np.concatenate([lens[frequent], [len_cls]])
    tree = _units(lv)
    assert tree == 1 << SZH_MAX_LEN, "Kraft: the frequent symbols and the class sum to %d / 2^24, not 1" % tree
    pow2 = rule["n_rare"] & (rule["n_rare"] - 1) == 0
    assert units <= 1 << SZH_MAX_LEN and (units == 1 << SZH_MAX_LEN) == pow2, "Kraft: all lengths sum to %d / 2^24 with %d rare symbols" % (units, rule["n_rare"])
    _held_to_optimum("the two-class book over the frequent counts and the class's weight %d" % rule["w_rare"], w, lv, L, fig)
    assert rule["rare_true"] * 48 <= total, "licence: %d rare occurrences of %d: more than 1/48" % (rule["rare_true"], total)
    return fig
