#!/usr/bin/env python3
"""seeded sweep over the SAMPLED-BOOK Lorenzo path: arrays of 2^22 .. 6.5e6 elements (the path starts at 2^22) at the
extents where stage 1's tasks of 256 x 4 rows x 16 planes (256 x 1 x 16 for 1-D arrays) end ragged, f32 and f64, eight kinds of data, every
payload held to the numpy model IN FULL (tests/payload_checks.py, tests/sampled_model.py) and then to every other form of the path byte for byte.
Per case (np.random.default_rng(SEED); every draw is made before anything runs on a device and depends on no device result):
  premises  from the model alone, before any launch and in DRY: one-byte codes, the class of the listed deltas, whether the 16-bit form of
            stage 1 is licensed and whether it voids its launch, whether the book is sampled. A case is never skipped: a device that
            disagrees with a premise is a failure.
  A  a fresh context sized to the sweep's largest array: the first payload — stage-1 codes, both lists, header, the book against the
     sample's counts (check_book), chunkwords and restart offsets of all chunks, the slow decoder on up to nine chunks (first, last, densest,
     first of offset group 1, last of the last full group, one with an escape, three drawn), the decode bit for bit against the model.
  B  the context's second and third call, three drawn encoder settings, the same context after the previous case's array (another shape,
     another book): the first payload's bytes. dc.q16 and spec_stats as the model has them; one drawn decoder form: the same array.
One case in five is a NEIGHBOUR that must not take the sampled book (n = 2^22 - 256, an x of 260 / 516, a 4-D array, quantbinCnt 128) and passes
every other check all the same (header esc_sym 0, version 4). Two fixed 1-D cases of n = 2^22 + 768 belong to every seed: exactly 2048 and
exactly 2049 listed deltas (steps of +-0.5), either side of what the packer's sort roles take.
Environment: SEED, N (drawn cases; the fixed two come on top), CASES=0,3 (only those run; all draws are still made; the fixed cases are -2 and
-1), VERBOSE, DRY=1 (no device call: draws, fields and premises). One line per failure with the case's tag, a tally, a line TALLY <json>, a
last line "cases ... failures K"; exit status 1 if K > 0, 2 after an error of the HIP runtime (nothing more runs on the device then)."""
import json, os, sys, time
from collections import Counter
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import sz3_amd
import szh_ref
import sampled_model as SM
import payload_checks

Dbg, Dbg2 = sz3_amd.Dbg, sz3_amd.Dbg2
LO, HI = 1 << 22, 6_500_000
X_EDGE = [256, 512, 768, 1024, 1280, 2048, 2560, 4096, 8192]
Y_EDGE = [2, 3, 5, 6, 7, 9, 61, 127, 203, 241, 911, 1093]
BOUNDS = [1e-2, 1e-3, 3e-4]
QBINS = [256, 1024, 65536]
KINDS = ["smooth", "c2", "rough", "constant", "listed-few", "listed-many", "nonfinite", "far-value"]
NEIGHBOURS = ["short", "x260", "4d", "radius64"]
ENCODER = ["K1_NO_Q16", "K1_NO_SAMP_IN_LAUNCH", "K1_Q16_PLAIN_STORES", "K1_NO_XCD_ORDER", "K1_NO_DEFER_FOLD", "CTX_NO_MEMORY", "PACK_SCAN_LAUNCH", "no-speculation"]
DECODER = ["DEC_NO_FUSED_X", "DEC_NO_HALF", "DEC_CARRY_PASS"]
LISTED = {"smooth": "none", "c2": "none", "constant": "none", "listed-few": "few", "listed-many": "many", "steps-2048": "few", "steps-2049": "many"}
EHIP = -4


class HipDown(Exception):
    """an error of the HIP runtime: the sweep ends, nothing more is started on the device"""


# ---- the draws -----------------------------------------------------------------------------------------------------------------------------------
def fit(rng, per, want=None, lo=LO, hi=HI):
    """an extent e with lo <= e * per <= hi, e >= 2; want: a predicate the extent should meet if one in the window does. None: no such extent"""
    a, b = max(2, -(-lo // per)), hi // per
    if b < a:
        return None
    cand = np.arange(a, b + 1)
    if want is not None and want(cand).any():
        cand = cand[want(cand)]
    return int(cand[int(rng.integers(0, len(cand)))])


def draw_shape(rng, rank):
    """a shape that takes the sampled book, from the edge lists"""
    while True:
        if rank == 1:
            odd = 2 * int(rng.integers(1, 4400)) + 1
            return (int([LO, LO + 256, LO + 256 * odd][int(rng.integers(0, 3))]),)
        if rank == 2:
            if rng.random() < 1 / 6:  # a two-row array
                return (2, 256 * int(rng.integers(8192, 12600)))
            x, r = int(rng.choice(X_EDGE)), int(rng.integers(0, 4))
            rows = fit(rng, x, lambda c: c % 4 == r)
            if rows is not None:
                return (rows, x)
        else:
            x, y = int(rng.choice(X_EDGE)), int(rng.choice(Y_EDGE))
            r = [0, 1, 15, None][int(rng.integers(0, 4))]
            z = fit(rng, x * y, None if r is None else (lambda c: c % 16 == r))
            if z is not None:
                return (z, y, x)


def draw_neighbour(rng, flavour):
    """-> (shape, quantbinCnt or None) of a case next to the sampled book's rule that must not take it"""
    if flavour == "short":
        return (LO - 256,), None
    if flavour == "x260":
        while True:
            x, y = int(rng.choice([260, 516])), int(rng.choice(Y_EDGE))
            z = fit(rng, x * y)
            if z is not None:
                return (z, y, x), None
    if flavour == "4d":
        while True:
            w, x, y = int(rng.integers(2, 4)), int(rng.choice([256, 512])), int(rng.choice(Y_EDGE[:8]))
            z = fit(rng, w * x * y)
            if z is not None:
                return (w, z, y, x), None
    return draw_shape(rng, int(rng.choice([2, 3]))), 128


def draw_case(rng, k, kind):
    c = {"k": k, "kind": kind}
    neighbour = rng.random() < 0.2
    flavour = NEIGHBOURS[int(rng.integers(0, 4))]
    if flavour == "radius64" and kind == "rough":  # (a rough field at radius 64 lists two values in a hundred: another stream altogether)
        flavour = "x260"
    rank = int(rng.choice([1, 2, 3, 3]))
    shape = draw_shape(rng, rank)
    nshape, nq = draw_neighbour(rng, flavour)
    c["neighbour"] = flavour if neighbour else None
    c["shape"] = nshape if neighbour else shape
    c["dtype"] = "float64" if rng.random() < 0.5 else "float32"
    c["eb"] = BOUNDS[int(rng.integers(0, 3))]
    qb = QBINS[int(rng.integers(0, 3))]
    c["qb"] = nq if (neighbour and nq) else qb
    c["field_seed"] = int(rng.integers(1, 1 << 30))
    c["rough_steps"] = float(rng.uniform(20.0, 28.0))
    c["encoder"] = [ENCODER[int(i)] for i in rng.choice(len(ENCODER), 3, replace=False)]
    c["decoder"] = DECODER[int(rng.integers(0, 3))]
    c["chunks"] = [int(v) for v in rng.integers(0, 1 << 30, 3)]
    return c


def fixed_case(seed, which, rng):
    """the two 1-D cases of every seed: exactly 2048 / 2049 steps of +-0.5, a listed delta each"""
    steps = 2048 + which
    return {"k": which - 2, "kind": "steps-%d" % steps, "neighbour": None, "shape": (LO + 768,), "dtype": "float32" if (seed + which) % 2 == 0 else "float64",
            "eb": 1e-3, "qb": 65536, "field_seed": 1000 + seed, "rough_steps": 0.0, "steps": steps,
            "encoder": [ENCODER[int(i)] for i in rng.choice(len(ENCODER), 3, replace=False)], "decoder": DECODER[int(rng.integers(0, 3))],
            "chunks": [int(v) for v in rng.integers(0, 1 << 30, 3)]}


def draw_all(seed, n_cases):
    rng = np.random.default_rng(seed)
    kinds = [KINDS[int(i)] for i in rng.permutation(len(KINDS))]
    cases = [fixed_case(seed, 0, rng), fixed_case(seed, 1, rng)]
    return cases + [draw_case(rng, k, kinds[k % len(kinds)]) for k in range(n_cases)]


def tag_of(c, seed):
    return "case %d (SEED %d) %s %s %s eb %g quantbinCnt %d%s; encoder %s, decoder %s" % (
        c["k"], seed, "x".join(map(str, c["shape"])), c["dtype"], c["kind"], c["eb"], c["qb"], " NEIGHBOUR %s" % c["neighbour"] if c["neighbour"] else "",
        "+".join(c["encoder"]), c["decoder"])


# ---- the fields ----------------------------------------------------------------------------------------------------------------------------------
def base_field(shape, sigma, seed, amp=1.0):
    """float64: the benchmark's fields by rank (tests/fields.py) — rank 1 a slow sine: a flattened volume is no smooth 1-D array. (The waves are
    evaluated in float32 on phases reduced in integers first: a third of the time, and the model is made from the array as it comes out.)"""
    ax = [np.arange(s, dtype=np.int32) for s in shape]
    two_pi = np.float32(2 * np.pi)
    wave = lambda f, k, period: f(two_pi * ((k % period).astype(np.float32) / np.float32(period)))  # noqa: E731
    if len(shape) == 1:
        f = wave(np.sin, ax[0], 4096) + np.float32(0.25) * wave(np.sin, ax[0], 1237)
    elif len(shape) == 2:
        y, x = ax[0][:, None], ax[1][None, :]
        f = wave(np.sin, x, 64) * wave(np.cos, y, 96) + np.float32(0.25) * wave(np.sin, x + 2 * y, 37)
    elif len(shape) == 3:
        z, y, x = ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]
        f = wave(np.sin, x, 64) * wave(np.cos, y, 96) * wave(np.sin, z, 128) + np.float32(0.25) * wave(np.sin, x + 2 * y + 3 * z, 37)
    else:
        t, z, y, x = ax[0][:, None, None, None], ax[1][None, :, None, None], ax[2][None, None, :, None], ax[3][None, None, None, :]
        f = wave(np.sin, 2 * x + t, 64) * wave(np.cos, y, 48) * wave(np.sin, z, 64) * (1 + np.float32(0.01) * t.astype(np.float32))
    f = amp * np.array(np.broadcast_to(f, shape), dtype=np.float64, order="C")
    if sigma:
        f += sigma * np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)
    return f


def clear_places(shape, count, rng):
    """`count` distinct flat indices none of whose Lorenzo stencils (the element and its neighbours one step up along every subset of the axes)
    touches a window of the probe: what is put there the probe does not see"""
    n = int(np.prod(shape))
    strides = [int(np.prod(shape[i + 1:])) for i in range(len(shape))]
    offs = [0]
    for s in strides:
        offs += [o + s for o in offs]
    cand = np.unique(rng.integers(0, n, 2 * count + 64))
    ok = np.ones(cand.size, dtype=bool)
    for o in offs:
        p = cand + o
        ok &= (p >= n) | (p % SM.PROBE_STRIDE >= SM.PROBE_RUN)
    cand = rng.permutation(cand[ok])
    assert cand.size >= count
    return np.sort(cand[:count])


def field_of(c):
    shape, T, eb, kind = c["shape"], np.dtype(c["dtype"]), c["eb"], c["kind"]
    rng = np.random.default_rng(c["field_seed"])
    rank = len(shape)
    if kind == "constant":
        return np.full(shape, 0.0437, dtype=T)  # (no multiple of half a lattice step at any of the bounds: 2.2, 21.9, 72.8 steps)
    # rough: a noise whose Lorenzo deltas have a deviation of 20 .. 28 lattice steps (2-D at a bound of 1e-3: sigma 0.02 .. 0.028) — beyond that
    # one delta in 4096 passes +-127 and the stream takes two-byte codes
    sigma = 0.0 if kind == "smooth" else c["rough_steps"] * 2 * eb / 2 ** (rank / 2) if kind == "rough" else 2e-3
    # (rank >= 2 at the bound 3e-4: the wave of period 64 along x climbs 233 lattice steps per element on the array's first row, where the
    # Lorenzo stencil has no row below to cancel it, and the probe's first window lies there. The wave is scaled with the bound; the noise is not)
    a = base_field(shape, sigma, c["field_seed"], amp=min(1.0, eb / 1e-3) if rank >= 2 else 1.0)
    flat = a.reshape(-1)
    if kind.startswith("steps-"):  # a[c:] += v lists exactly one delta; c = 2048 j + 100 lies outside the probe's windows
        s = np.zeros(a.size)
        at = 2048 * np.arange(c["steps"]) + 100
        s[at] = np.where(np.arange(c["steps"]) % 2 == 0, 0.5, -0.5)
        flat += np.cumsum(s)
    if kind in ("listed-few", "listed-many"):  # spikes of 200 .. 900 lattice steps: 2^rank listed deltas each
        count = 30 if kind == "listed-few" else 2049 // 2 ** rank + 200
        at = clear_places(shape, count, rng)
        flat[at] += rng.choice([-1.0, 1.0], count) * rng.uniform(200, 900, count) * 2 * eb
    a = a.astype(T)
    flat = a.reshape(-1)
    if kind == "nonfinite":
        at = clear_places(shape, 6, rng)
        flat[at] = np.array([np.nan, np.inf, -np.inf, 1e30, np.nan, -1e30]).astype(T)
    if kind == "far-value":  # one value of 6000 lattice steps: beyond the 16-bit form of stage 1
        flat[clear_places(shape, 1, rng)] = T.type(6000 * 2 * eb)
    return a


# ---- the model: premises and expected values --------------------------------------------------------------------------------------------------
def model_of(c, a):
    """-> dict of everything the device must deliver, from numpy alone; raises AssertionError where a premise of the draw does not hold"""
    shape, eb, radius, n = c["shape"], c["eb"], c["qb"] // 2, a.size
    want_narrow = radius >= 128
    q, d, exp, bad, far = szh_ref.dualquant(a, eb, radius=radius, narrow=want_narrow)
    big, n_samples, one_byte = SM.probe(d)
    assert (radius >= 128 and one_byte) == want_narrow, "premise: one-byte codes (the probe meets %d far deltas of %d)" % (big, n_samples)
    sampled = SM.takes_sampled_book(shape, a.dtype, radius, n) and want_narrow
    assert sampled == (c["neighbour"] is None), "premise: the draw %s the sampled book" % ("takes" if sampled else "does not take")
    dout_idx = np.nonzero(far.reshape(-1))[0]
    vout_idx = np.nonzero(bad.reshape(-1))[0]
    cap = max(1024, n // 8)
    assert len(dout_idx) <= cap and len(vout_idx) <= cap, "premise: the lists hold what the stream lists"
    cls = "none" if len(dout_idx) == 0 else "few" if len(dout_idx) <= 2048 else "many"
    if c["kind"] in LISTED:
        assert cls == LISTED[c["kind"]], "premise: listed deltas of class %s (the model lists %d)" % (LISTED[c["kind"]], len(dout_idx))
    if c["kind"].startswith("steps-"):
        assert len(dout_idx) == c["steps"], "premise: exactly %d listed deltas (the model lists %d)" % (c["steps"], len(dout_idx))
    if c["kind"] == "nonfinite":
        alien = ~(np.abs(a.reshape(-1)) < 1e29)  # NaN, +-Inf, +-1e30
        assert alien.sum() == 6 and bad.reshape(-1)[alien].all(), "premise: six listed values that are no lattice points"
    m = dict(exp=exp.reshape(-1), dout_idx=dout_idx, dout_val=d.reshape(-1)[dout_idx].astype(np.int64), vout_idx=vout_idx, sampled=sampled, listed=cls,
             radius=radius, sample=SM.sample_counts(d, shape) if sampled else None, licensed=False, voids=False)
    if a.dtype == np.float32 and want_narrow:
        m["licensed"] = SM.q16_licensed(q, a, eb)
        m["voids"] = m["licensed"] and SM.q16_voids(a, eb)
    if c["kind"] in ("nonfinite", "far-value"):
        assert SM.q16_voids(a.astype(np.float32), eb), "premise: a value the 16-bit form does not take"
    return m


# ---- the device legs ---------------------------------------------------------------------------------------------------------------------------
def conf_of(shape, eb, qb):
    conf = sz3_amd.Config(*shape)
    conf.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
    conf.regression = 0
    conf.errorBoundMode = sz3_amd.EB_ABS
    conf.absErrorBound = eb
    conf.quantbinCnt = qb
    return conf


def guard(f):
    """an error of the HIP runtime ends the sweep; an assertion or a refusal is the case's failure"""
    try:
        return f()
    except sz3_amd.SZ3HipError as e:
        if e.code == EHIP:
            raise HipDown(str(e)[:300])
        raise AssertionError("refused: %s" % str(e)[:300])
    except RuntimeError as e:  # (torch's: a fault of an earlier launch surfaces here)
        raise HipDown(str(e)[:300])


def run_case(c, a, m, prev, T):
    """-> the failures of the case"""
    import torch
    dev = torch.device("cuda:0")
    bad = []
    conf = conf_of(c["shape"], c["eb"], c["qb"])
    t0 = time.time()
    t = torch.from_numpy(a).to(dev)
    dc = sz3_amd.DeviceCompressor(HI, a.dtype)
    cap = dc.payload_bound(HI, worst_case=True)
    pl = torch.empty(cap, dtype=torch.uint8, device=dev)
    c["times"]["context"] = round(time.time() - t0, 3)

    def call(tensor=t, cf=conf, setting=None):
        if setting == "no-speculation":
            dc.set_speculation(False)
        f1 = int(getattr(Dbg, setting)) if setting in Dbg.__members__ else 0
        f2 = int(getattr(Dbg2, setting)) if setting in Dbg2.__members__ else 0
        try:
            with sz3_amd.debug_flags(f1), sz3_amd.debug_flags2(f2):
                size = dc.compress(cf, tensor.data_ptr(), pl.data_ptr(), cap, 0)
        finally:
            if setting == "no-speculation":
                dc.set_speculation(True)
        return pl[:size].cpu().numpy().tobytes()

    def decode(blob_size, flags=0):
        out = torch.empty_like(t)
        with sz3_amd.debug_flags(int(flags)):
            dc.decompress(pl.data_ptr(), blob_size, out.data_ptr(), 0)
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

    # A: the first payload, in full
    first = leg("A, the first call", call)
    if first is None:
        return bad
    got = leg("A, codes and decode", lambda: (dc.debug_codes(a.size), dc.stats(), decode(len(first))))
    if got is None:
        return bad
    codes, st, dec = got

    def in_full():
        assert bool(st["narrow_codes"]) == (m["radius"] >= 128), "one-byte codes: %d, the model's probe says %d" % (st["narrow_codes"], m["radius"] >= 128)
        h, fig = payload_checks.check_payload(a, c["eb"], m["exp"], m["dout_idx"], m["dout_val"], m["vout_idx"], first, codes, st, dec, sample=m["sample"], extra_chunks=c["chunks"])
        assert h["radius"] == m["radius"]
        if not m["sampled"]:
            assert h["esc_sym"] == 0 and h["version"] == 4, "a neighbour took the sampled book (esc_sym %d, version %d)" % (h["esc_sym"], h["version"])
        elif fig["book"]["limit_binds"]:
            T["excess"][c["kind"]] = max(T["excess"].get(c["kind"], 0.0), fig["book"]["excess"])
            T["limit_binds"] += 1
    leg("A", in_full)

    # B: every other form writes those bytes
    def warm():
        for k in (2, 3):
            assert call() == first, "call %d of the context writes another payload" % k
            if m["sampled"]:
                want = m["licensed"] and not m["voids"]  # (a launch that voids itself keeps the following calls off the 16-bit form)
                assert dc.q16 == want, "call %d: q16 %d, the model licenses %d (probe %d, voids %d)" % (k, dc.q16, want, m["licensed"], m["voids"])
                assert dc.spec_stats()[1] == int(m["voids"]), "call %d: %d misses, the model has %d" % (k, dc.spec_stats()[1], int(m["voids"]))
    leg("B, later calls", warm)

    def under(s):
        assert call(setting=s) == first, "another payload"
    for s in c["encoder"]:
        leg("B, " + s, lambda s=s: under(s))

    def misses():
        assert dc.spec_stats()[1] == 0, "%d misses of the speculation" % dc.spec_stats()[1]
    if m["sampled"] and not m["voids"]:
        leg("B, misses", misses)
    if prev is not None:
        def history():
            pa, pc = prev
            tp = torch.from_numpy(np.ascontiguousarray(pa.astype(a.dtype))).to(dev)
            pconf = conf_of(pc["shape"], pc["eb"], pc["qb"])
            call(tp, pconf)
            assert call() == first, "the payload depends on what the context coded before"
        leg("B, after the previous case's array", history)

    def other_decoder():
        size = len(call())
        got = decode(size, getattr(Dbg, c["decoder"]))
        assert payload_checks.bits_equal(got, dec), "another array"
    leg("B, decoder " + c["decoder"], other_decoder)
    dc.close()
    return bad


def main():
    seed = int(os.environ.get("SEED", "1"))
    n_cases = int(os.environ.get("N", "4"))
    sel = set(int(x) for x in os.environ["CASES"].split(",")) if os.environ.get("CASES") else None
    verbose, dry = bool(os.environ.get("VERBOSE")), bool(os.environ.get("DRY"))
    T = {"rank": Counter(), "dtype_rank": Counter(), "kind": Counter(), "neighbour": Counter(), "encoder": Counter(), "decoder": Counter(), "y_mod_4": Counter(),
         "z_mod_16": Counter(), "listed": Counter(), "z_below_16": 0, "ragged_chunk": 0, "ragged_nseg": 0, "sampled": 0, "licensed": 0, "voids": 0,
         "limit_binds": 0, "excess": {}, "seconds": 0.0}
    failures = n_run = 0
    down = None
    prev = None
    t0 = time.time()
    if not dry:
        import torch  # noqa: F401
    for c in draw_all(seed, n_cases):
        if sel and c["k"] not in sel:
            continue
        n_run += 1
        shape = c["shape"]
        n = int(np.prod(shape))
        tag = tag_of(c, seed)
        if verbose:
            print(tag, flush=True)
        bad = []
        c["times"] = {}
        t1 = time.time()
        a = field_of(c)
        c["times"]["field"] = round(time.time() - t1, 3)
        t1 = time.time()
        try:
            m = model_of(c, a)
        except AssertionError as e:
            m = None
            bad.append(str(e)[:300])
        c["times"]["model"] = round(time.time() - t1, 3)
        if m is not None:
            T["kind"][c["kind"]] += 1
            T["neighbour"][str(c["neighbour"])] += 1
            for s in c["encoder"]:
                T["encoder"][s] += 1
            T["decoder"][c["decoder"]] += 1
            T["listed"][m["listed"]] += 1
            T["licensed"] += int(m["licensed"])
            T["voids"] += int(m["voids"])
            if m["sampled"]:  # (what the draws must cover is about the arrays that take the path)
                d3 = (1,) * (3 - len(shape)) + tuple(shape)
                T["sampled"] += 1
                T["rank"][str(len(shape))] += 1
                T["dtype_rank"]["%s/%d" % (c["dtype"], len(shape))] += 1
                if len(shape) >= 2:
                    T["y_mod_4"][str(d3[1] % 4)] += 1
                if len(shape) == 3:
                    T["z_mod_16"][str(d3[0] % 16)] += 1
                    T["z_below_16"] += int(d3[0] < 16)
                T["ragged_chunk"] += int(n % 1024 != 0)
                T["ragged_nseg"] += int((n // 256) % 1024 != 0)
            if not dry:
                try:
                    bad += run_case(c, a, m, prev, T)
                except HipDown as e:
                    bad.append("%s — the sweep ends here" % e)
                    down = e
                finally:
                    sz3_amd.lib().sz3hip_debug_flags(0)
                    sz3_amd.lib().sz3hip_debug_flags2(0)
        prev = (a, c)
        if verbose:
            print("  seconds: " + ", ".join("%s %.3f" % kv for kv in c["times"].items()), flush=True)
        for b in bad:
            failures += 1
            print("FAIL %s: %s" % (tag, b), flush=True)
        if down is not None:
            break
    T["seconds"] = round(time.time() - t0, 2)
    show = lambda cn: ", ".join("%s %d" % (k, cn[k]) for k in sorted(cn, key=str))  # noqa: E731
    print("sampled %d | rank: %s | dtype/rank: %s | neighbours: %s" % (T["sampled"], show(T["rank"]), show(T["dtype_rank"]), show(T["neighbour"])))
    print("kind: %s | listed deltas: %s | 16-bit form licensed %d, voided %d" % (show(T["kind"]), show(T["listed"]), T["licensed"], T["voids"]))
    print("y %% 4: %s | z %% 16: %s | z < 16: %d | n %% 1024 != 0: %d | nseg %% 1024 != 0: %d" % (show(T["y_mod_4"]), show(T["z_mod_16"]), T["z_below_16"], T["ragged_chunk"], T["ragged_nseg"]))
    print("encoder settings: %s | decoder forms: %s" % (show(T["encoder"]), show(T["decoder"])))
    if not dry:
        print("books bound by the 16-bit limit: %d; largest excess over package-merge in bits per sampled symbol, by kind: %s" % (T["limit_binds"], json.dumps(T["excess"], sort_keys=True)))
    print("TALLY " + json.dumps({k: (dict(v) if isinstance(v, Counter) else v) for k, v in T.items()}, sort_keys=True))
    print("cases %d (SEED %d, %s) failures %d" % (n_run, seed, "DRY: draws and premises only" if dry else "on the device", failures))
    sys.exit(2 if down is not None else 1 if failures else 0)


if __name__ == "__main__":
    main()
