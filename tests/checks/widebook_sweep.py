#!/usr/bin/env python3
"""seeded sweep over the WIDE code books: drawn histograms of 300 .. 65 535 symbols, shown to the Huffman stage as
arrays whose two-byte code stream has exactly those counts (tests/crafted_codes.py, the balanced order), every payload held to the numpy model
IN FULL (tests/payload_checks.py, tests/widebook_model.py) and then to other forms of the path byte for byte.
Per case (np.random.default_rng(SEED); every draw is made before anything runs on a device and depends on no device result):
  histogram  m symbols — half of the draws at a boundary of the constructions or one next to it (641, 3840 / 3841, 4096 / 4097, 15360 /
             15361, 16384 / 16385, 65535), the others log-uniform over 641 .. 65535 — in one of the shapes flat, geometric, Zipf, two-tier
             (a head for tier 1 or tier 2 over a tail of equal counts: floor engaged or not, 2^k rare symbols or not), Fibonacci tail (1100 ..
             1200 symbols, a tree deeper than 24 bits), sparse-short (300 .. 512 symbols 16 bins apart: the wide path under the 16-bit limit,
             flat or Fibonacci); symbols 1 or — where m allows — 4 bins apart; 50 K .. 1.5 M elements; f32 or f64.
  premises   from the model alone, before any launch and in DRY: the array codes to the prescribed stream (assert_prescribed), the path is the
             wide book's, a book that keeps every rule exists (model_lens / check_wide_book). A case is never skipped.
  A  a fresh context's first call: check_payload in full — codes, lists (none), header, the book against widebook_model, the chunk table, the
     slow decoder on the picked chunks (the one with the most rare-class symbols among them), the decode bit for bit.
  B  the context's second call, one drawn encoder form (CB_COMPACT_IN_WG, CB_NO_SPEC_WIDE, CTX_NO_MEMORY, CB_SERIAL_MERGE, no speculation) on a
     context of its own: the first payload's bytes. One drawn decoder form: the same array.
Stage 1 keeps one-byte codes where its probe meets few far deltas; where the model of the probe says so the case runs under K1_NO_NARROW, and
every case asserts two-byte codes.
Environment: SEED, N, CASES=0,3 (only those run; all draws are still made), VERBOSE, DRY=1 (no device call: draws, arrays and premises). One
line per failure, a tally, a line TALLY <json>, a last line "cases ... failures K"; exit status 1 if K > 0, 2 after an error of the HIP
runtime (nothing more runs on the device then)."""
import json, os, sys, time
from collections import Counter
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import crafted_codes as cc
import payload_checks
import sampled_model
import szh_ref
import widebook_model as wm

BOUNDARY = [641, 642, 3840, 3841, 4096, 4097, 4098, 15360, 15361, 16384, 16385, 65534, 65535]
KINDS = ["flat", "geometric", "zipf", "two-tier", "fib-tail", "sparse-short"]
TIERS = ["t1-floor", "t1-heavy", "t1-pow2", "t2", "t2-pow2"]
ENCODER = ["CB_COMPACT_IN_WG", "CB_NO_SPEC_WIDE", "CTX_NO_MEMORY", "CB_SERIAL_MERGE", "no-speculation"]
DECODER = ["DEC_NO_FUSED_X", "DEC_NO_HALF", "DEC_CARRY_PASS"]
N_LO, N_HI = 50_000, 1_500_000
EHIP = -4


class HipDown(Exception):
    """an error of the HIP runtime: the sweep ends, nothing more is started on the device"""


# ---- the draws -----------------------------------------------------------------------------------------------------------------------------------
def _scaled(w, n):
    """integer counts >= 1 in the proportions of w whose sum is about n"""
    w = np.asarray(w, dtype=np.float64)
    return np.maximum(1, np.rint(w * (n / w.sum()))).astype(np.int64)


def _fib_upto(lo, total):
    """Fibonacci numbers from the first one >= lo on, as many as sum to at most `total`"""
    out, a, b = [], 1, 2
    while a < lo:
        a, b = b, a + b
    while sum(out) + a <= total:
        out.append(a)
        a, b = b, a + b
    return out


def draw_case(rng, k):
    kind = KINDS[int(rng.integers(len(KINDS)))]
    n = int(np.exp(rng.uniform(np.log(N_LO), np.log(N_HI))))
    m = int(BOUNDARY[int(rng.integers(len(BOUNDARY)))]) if rng.random() < 0.5 else int(np.exp(rng.uniform(np.log(641), np.log(65535))))
    sub, spacing = None, 1
    if kind == "flat":
        n = max(n, m)
        counts = np.full(m, n // m, dtype=np.int64)
    elif kind == "geometric":
        n = max(n, 2 * m)
        counts = _scaled(float(rng.choice([30.0, 1000.0, 1e5])) ** (-np.arange(m) / float(m - 1)), n)
    elif kind == "zipf":
        n = max(n, 2 * m)
        counts = _scaled(1.0 / np.arange(1, m + 1) ** float(rng.choice([0.8, 1.0, 1.4])), n)
    elif kind == "two-tier":
        sub = TIERS[int(rng.integers(len(TIERS)))]
        t2 = sub.startswith("t2")
        floor_at = 15360 if t2 else 4096   # m must exceed keep + keep / 4, and CB_CLASS_MIN
        if sub == "t1-floor":  # 1100 .. 1200 rare occurrences of 1.3 M: 11 index bits, the floor is total >> 10
            head, tail, hi, lo = int(rng.integers(3000, 3073)), int(rng.integers(1100, 1200)), 1200.0, 100.0
        else:
            head = int(rng.integers(9000, 12289)) if t2 else int(rng.integers(2000, 3073))
            tail = (8192 if t2 else 4096) if sub.endswith("pow2") else int(rng.integers(floor_at - head + 1, floor_at - head + 3000))
            hi, lo = (200.0, 70.0) if t2 else (2000.0, 40.0)
        each = 3 if sub == "t1-heavy" else 1
        counts = np.concatenate([np.rint(hi * (lo / hi) ** (np.arange(head) / float(head - 1))).astype(np.int64), np.full(tail, each, dtype=np.int64)])
        if t2:
            counts[0] = int(rng.integers(50_000, 200_000))
    elif kind == "fib-tail":
        m = int(rng.integers(1100, 1201))  # (a body of 1086 .. 1186 symbols met once: a subtree 11 levels deep; 14 terms from 987 on above it)
        chain = _fib_upto(987, N_HI - m)
        counts = np.concatenate([np.ones(m - len(chain), dtype=np.int64), np.array(chain, dtype=np.int64)])
    else:  # sparse-short
        m = int(rng.choice([300, 511, 512, int(rng.integers(257, 513))]))
        spacing = 16
        n = min(n, 100_000)   # (equal counts 16 bins apart: the deltas' sum, 8 m * count, must stay on the lattice)
        if rng.random() < 0.5:
            counts = np.full(m, max(1, n // m), dtype=np.int64)
        else:
            # (tests/crafted_codes.py's sparse-fib16 at the drawn size: twelve Fibonacci terms, each heavier than the whole body below them —
            # a tree five levels deeper than 16 bits, where the 16-bit optimum itself keeps the project's 0.2 % rule)
            counts = np.concatenate([np.full(m - 12, 3, dtype=np.int64), 4 * (m - 12) * np.array(cc._fib(12), dtype=np.int64)])
    m = len(counts)
    if spacing == 1 and 4 * m <= 65535 and rng.random() < 1 / 3.0:
        spacing = 4
    return dict(k=k, kind=kind, sub=sub, m=m, spacing=spacing, counts=counts, dtype=("f32", "f64")[int(rng.integers(2))], seed=int(rng.integers(1, 1 << 30)),
                encoder=ENCODER[int(rng.integers(len(ENCODER)))], decoder=DECODER[int(rng.integers(len(DECODER)))])


def draw_all(seed, n_cases):
    rng = np.random.default_rng(seed)
    return [draw_case(rng, k) for k in range(n_cases)]


def tag_of(c, seed):
    return "SEED=%d k=%d %s%s m=%d spacing=%d n=%d %s enc=%s dec=%s" % (seed, c["k"], c["kind"], "/" + c["sub"] if c["sub"] else "", c["m"], c["spacing"],
                                                                      int(c["counts"].sum()), c["dtype"], c["encoder"], c["decoder"])


def histogram_of(c):
    """-> (freq over [sym_min, sym_max], sym_min)"""
    sym = cc.deltas_by_count(c["counts"]) * c["spacing"] + cc.RADIUS
    freq = np.zeros(int(sym.max() - sym.min()) + 1, dtype=np.int64)
    freq[sym - sym.min()] = c["counts"]
    return freq, int(sym.min())


def regime_of(c):
    """what the model says of the case's histogram (no array needed) -> dict"""
    freq, sym_min = histogram_of(c)
    rule = wm.class_rule(freq)
    w = freq[freq > 0] if rule is None else wm.class_weights(freq, rule)[0]
    L = wm.limit(c["m"])
    return dict(path=wm.path(freq), limit=L, rule=rule, mk=len(w), binds=szh_ref.huffman_cost(w)[1] > L)


def array_of(c):
    d = cc.delta_stream(c["counts"], "balanced", seed=c["seed"], spacing=c["spacing"])
    return cc.array_from_deltas(d, np.float32 if c["dtype"] == "f32" else np.float64)


def model_of(c, x, exp):
    """the premises; -> regime_of's dict + the base flags"""
    cc.assert_prescribed(x, exp)
    freq, sym_min = histogram_of(c)
    assert np.array_equal(np.bincount(exp, minlength=65536)[sym_min:sym_min + len(freq)], freq) and x.size == freq.sum()
    r = regime_of(c)
    assert r["path"] != wm.SMALL, "the histogram is cb_small's: not a case of this sweep"
    wm.check_wide_book(wm.model_lens(freq), freq, sym_min)   # a book that keeps every rule exists (the two-class form does not fall back)
    r["narrow"] = bool(sampled_model.narrow_codes(exp.astype(np.int64) - cc.RADIUS, cc.RADIUS))
    return r


def tally(T, c, r):
    rule = r["rule"]
    T["kind"][c["kind"] + ("/" + c["sub"] if c["sub"] else "")] += 1
    T["dtype"][c["dtype"]] += 1
    T["spacing"][str(c["spacing"])] += 1
    T["encoder"][c["encoder"]] += 1
    T["decoder"][c["decoder"]] += 1
    T["one_class_below_4097"] += int(c["m"] <= wm.CB_CLASS_MIN)
    T["both_tiers_rejected"] += int(c["m"] > wm.CB_CLASS_MIN and rule is None)
    T["tier1"] += int(rule is not None and rule["keep"] == wm.CB_CLASS_KEEP)
    T["tier2"] += int(rule is not None and rule["keep"] == wm.CB_CLASS_KEEP2)
    T["floor_engaged"] += int(rule is not None and rule["floor_engaged"])
    T["floor_not_engaged"] += int(rule is not None and not rule["floor_engaged"])
    T["n_rare_pow2"] += int(rule is not None and rule["n_rare"] & (rule["n_rare"] - 1) == 0)
    T["mk_beyond_lds"] += int(r["mk"] > wm.CB_LDS_KEYS)
    T["limit_16_wide"] += int(r["limit"] == 16)
    T["limit_binds"] += int(r["binds"])
    T["at_boundary"] += int(c["m"] in BOUNDARY)


# ---- the device -------------------------------------------------------------------------------------------------------------------------------
def guard(f):
    import sz3_amd
    try:
        return f()
    except sz3_amd.SZ3HipError as e:
        if e.code == EHIP:
            raise HipDown(str(e)[:300])
        raise AssertionError("refused: %s" % str(e)[:300])
    except RuntimeError as e:  # (torch's: a fault of an earlier launch surfaces here)
        raise HipDown(str(e)[:300])


def run_case(c, x, exp, r, T):
    """-> the failures of the case"""
    import torch
    import sz3_amd
    Dbg = sz3_amd.Dbg
    dev = torch.device("cuda:0")
    bad = []
    conf = sz3_amd.Config(*x.shape)
    conf.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
    conf.regression = 0
    conf.errorBoundMode = sz3_amd.EB_ABS
    conf.absErrorBound = cc.EB
    t = torch.from_numpy(x).to(dev)
    base = int(Dbg.K1_NO_NARROW) if r["narrow"] else 0
    ctx = {}

    def context():
        dc = sz3_amd.DeviceCompressor(x.size, x.dtype)
        cap = dc.payload_bound(x.size, worst_case=True)
        return dc, cap, torch.empty(cap, dtype=torch.uint8, device=dev)

    def call(dcp, flags=0):
        dc, cap, pl = dcp
        with sz3_amd.debug_flags(int(flags) | base):
            size = dc.compress(conf, t.data_ptr(), pl.data_ptr(), cap, 0)
        return pl[:size].cpu().numpy().tobytes()

    def decode(dcp, size, flags=0):
        dc, cap, pl = dcp
        out = torch.empty_like(t)
        with sz3_amd.debug_flags(int(flags)):
            dc.decompress(pl.data_ptr(), size, out.data_ptr(), 0)
            torch.cuda.synchronize()
        return out.cpu().numpy()

    def leg(name, f):
        t0 = time.time()
        try:
            return guard(f)
        except (AssertionError, ValueError, IndexError, KeyError) as e:  # (the slow decoder answers a broken stream with a ValueError)
            bad.append("leg %s: %s%s" % (name, "" if isinstance(e, AssertionError) else type(e).__name__ + ": ", str(e)[:300]))
        finally:
            c["times"][name] = round(time.time() - t0, 3)
        return None

    def first_call():
        ctx["a"] = context()
        return call(ctx["a"])
    first = leg("A, the first call", first_call)
    if first is None:
        return bad
    got = leg("A, codes and decode", lambda: (ctx["a"][0].debug_codes(x.size), ctx["a"][0].stats(), decode(ctx["a"], len(first))))
    if got is None:
        return bad
    codes, st, dec = got

    def in_full():
        assert st["narrow_codes"] == 0, "one-byte codes: not the wide book's stream"
        none = np.zeros(0, dtype=np.int64)
        h, fig = payload_checks.check_payload(x, cc.EB, exp, none, none, none, first, codes, st, dec)
        w = fig["wide"]
        assert w is not None and (w["rule"] is None) == (r["rule"] is None) and w["limit_binds"] == r["binds"]
        if w["limit_binds"]:
            T["over_pm"][c["kind"]] = max(T["over_pm"].get(c["kind"], 0.0), (w["cost"] - w["pm_cost"]) / float(x.size))
        if w["two_class"]:
            T["over_one_class"][c["kind"] + "/" + str(c["sub"])] = max(T["over_one_class"].get(c["kind"] + "/" + str(c["sub"]), 0.0), w["over_one_class"])
    leg("A", in_full)

    def again():
        assert call(ctx["a"]) == first, "the context's second call writes another payload"
    leg("B, second call", again)

    def under():
        other = context()
        if c["encoder"] == "no-speculation":
            other[0].set_speculation(False)
            assert call(other) == first and call(other) == first, "another payload"
        else:
            f = int(getattr(Dbg, c["encoder"]))
            assert call(other, f) == first and call(other, f) == first, "another payload"
        other[0].close()
    leg("B, " + c["encoder"], under)

    def other_decoder():
        size = len(call(ctx["a"]))
        assert payload_checks.bits_equal(decode(ctx["a"], size, getattr(Dbg, c["decoder"])), dec), "another array"
    leg("B, decoder " + c["decoder"], other_decoder)
    ctx["a"][0].close()
    return bad


def main():
    seed = int(os.environ.get("SEED", "1"))
    n_cases = int(os.environ.get("N", "6"))
    sel = set(int(v) for v in os.environ["CASES"].split(",")) if os.environ.get("CASES") else None
    verbose, dry = bool(os.environ.get("VERBOSE")), bool(os.environ.get("DRY"))
    T = {k: Counter() for k in ("kind", "dtype", "spacing", "encoder", "decoder")}
    T.update({k: 0 for k in ("one_class_below_4097", "both_tiers_rejected", "tier1", "tier2", "floor_engaged", "floor_not_engaged", "n_rare_pow2", "mk_beyond_lds",
                             "limit_16_wide", "limit_binds", "at_boundary")})
    T.update(over_pm={}, over_one_class={}, seconds=0.0)
    failures = n_run = 0
    down = None
    t0 = time.time()
    for c in draw_all(seed, n_cases):
        if sel and c["k"] not in sel:
            continue
        n_run += 1
        tag = tag_of(c, seed)
        if verbose:
            print(tag, flush=True)
        bad = []
        c["times"] = {}
        t1 = time.time()
        r = None
        try:
            x, exp = array_of(c)
            c["times"]["array"] = round(time.time() - t1, 3)
            t1 = time.time()
            r = model_of(c, x, exp)
        except AssertionError as e:
            bad.append("premise: " + str(e)[:300])
        c["times"]["model"] = round(time.time() - t1, 3)
        if r is not None:
            tally(T, c, r)
            if not dry:
                import sz3_amd
                try:
                    bad += run_case(c, x, exp, r, T)
                except HipDown as e:
                    bad.append("%s — the sweep ends here" % e)
                    down = e
                finally:
                    sz3_amd.lib().sz3hip_debug_flags(0)
        if verbose:
            print("  seconds: " + ", ".join("%s %.3f" % kv for kv in c["times"].items()), flush=True)
        for b in bad:
            failures += 1
            print("FAIL %s: %s" % (tag, b), flush=True)
        if down is not None:
            break
    T["seconds"] = round(time.time() - t0, 2)
    show = lambda cn: ", ".join("%s %d" % (k, cn[k]) for k in sorted(cn, key=str))  # noqa: E731
    print("kind: %s | dtype: %s | spacing: %s" % (show(T["kind"]), show(T["dtype"]), show(T["spacing"])))
    print("one class below 4097 symbols %d, both tiers rejected %d, tier 1 %d, tier 2 %d | floor engaged %d, not %d | 2^k rare symbols %d | more than 16384 keys %d | "
          "16-bit limit %d | limit binds %d | at a boundary %d" % tuple(T[k] for k in ("one_class_below_4097", "both_tiers_rejected", "tier1", "tier2", "floor_engaged",
                                                                                       "floor_not_engaged", "n_rare_pow2", "mk_beyond_lds", "limit_16_wide", "limit_binds", "at_boundary")))
    print("encoder forms: %s | decoder forms: %s" % (show(T["encoder"]), show(T["decoder"])))
    if not dry:
        print("bits per symbol over package-merge where the limit binds, by kind: %s; of the two-class book over the one-class unlimited code: %s" % (
            json.dumps(T["over_pm"], sort_keys=True), json.dumps(T["over_one_class"], sort_keys=True)))
    print("TALLY " + json.dumps({k: (dict(v) if isinstance(v, Counter) else v) for k, v in T.items()}, sort_keys=True))
    print("cases %d (SEED %d, %s) failures %d" % (n_run, seed, "DRY: draws and premises only" if dry else "on the device", failures))
    sys.exit(2 if down is not None else 1 if failures else 0)


if __name__ == "__main__":
    main()
