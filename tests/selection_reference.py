"""fp64 restatement of the adaptive selection (stage A4) under the sampler's transform, and a checker that excuses no ray.

losses[0] = BCEWithLogitsLoss / CrossEntropyLoss makes the selection kernels compute a sigmoid / a softmax over the 128 bins before
they compare and rank: from then on the selection is floating-point code and cannot be pinned bit for bit against a reference that
uses another expf or another summation order.  What can be pinned:

  transform64      the transform in float64 on the kernel's own fp32 inputs (softmax: row maximum subtracted; NaN / inf as IEEE gives them)
  transform_bound  a RELATIVE bound on a transformed value: twice the largest relative residual of the fp32 numpy restatement
                   (adanerf_oracle.oracle_transform) against transform64 on the same rows -- the samplers' rule of
                   stage_reference.sampler_bound.  The factor two covers the <= 1 ulp between numpy's expf and the device's and the other
                   summation order of the softmax.  Measured against the reference only, never against a kernel.  FLOOR = 2^-126 is
                   added as an absolute term (fp32 results below the normal range carry no relative accuracy).
  check_selection  with v = transform64, e_j = bound |v_j| + FLOOR (0 where v_j is infinite) and thr = float32(thr), every ray must carry
                   an eps-valid selection:
     shape      1 <= count <= n_max, bins strictly ascending in 0..127
     values     every kept value within e of v at its bin; an infinite v matched exactly
     regular    every kept bin has v >= thr - e; count < n_max: every left-out number has v < thr + e; count = n_max: every left-out
                number has v < thr + e or v - e <= min over the kept bins of (v + e)
     fallback   (instead of regular) count = 1, the kept v < thr - e, every number < thr + e, the kept v within e of the largest
     NaN        never ranks: no kept bin has a NaN v, unless the whole row is NaN (also a softmax row holding a NaN or a +inf) -- that
                row keeps bin 0 alone, its kept value a NaN
     ties       no tolerance: a left-out bin j and a kept bin k > j whose inputs are equal numbers.  Equal inputs give equal transformed
                values in any deterministic kernel, so "lower bin first" survives every transform.  Under the sigmoid two more
                classes are equal whatever expf's last bit is (tie_keys): logits >= 18 are exactly 1.0f in fp32 (sigmoid(18) =
                1 - 1.5e-8, less than half an ulp below 1; in the kernel's form 1 + expf(-x) rounds to 1), logits <= -104 are exactly 0
                (6.8e-46 is less than half the smallest denormal; expf(104) overflows).
     margin     the rays decided with margin -- every |v_j - thr| > 2 e_j, and at the cut-off (count limited by n_max, or the fallback's
                arg-max) either a gap > 2 e or a tie of equal inputs whose value is > 2 e away from every other value -- must ALSO equal
                the fp64 set rule exactly.  Nothing is excused on the other rays: the eps-rule still binds them.
  selection_inputs about 1 000 rows per transform: random rows (own scale in [0.3, 3] and offset in [-3, 1] each), quantised rows (six
                   levels: many equal logits), determinate edge rows with their expected bins.
  guard_inputs / guard_classes / check_guarded
                   the guarded two-precision selection under every transform: inputs within a raw band of each other, the float64 classes
                   "undecided for every / for some correct fp32 kernel", and what a device result owes -- see the section at the end.

numpy only."""
import numpy as np

import adanerf_oracle as O

F32 = np.float32
FLOOR = 2.0 ** -126
SOFTMAX = ("CrossEntropyLoss", "CrossEntropyLossWeighted")
LOSSES = ("MSE", "BCEWithLogitsLoss", "CrossEntropyLoss")
# the threshold each transform is used with, and the three thresholds that sit exactly on values the edge rows produce
THRESHOLDS = {"MSE": 0.2, "BCEWithLogitsLoss": 0.6, "CrossEntropyLoss": 0.012}
BOUNDARY = (0.5, 1.0 / 128.0, float(np.nextafter(F32(1.0 / 128.0), F32(1.0))))
SIGMOID_ONE, SIGMOID_ZERO = 18.0, -104.0      # see "ties" above
LEVELS = np.array([-4.0, -1.5, 0.0, 0.5, 2.0, 5.0], F32)      # quantised rows; raw 0.5 and sigmoid(0) = 0.5 sit on the threshold 0.5 on purpose


def transform64(raw, losses0):
    x = np.asarray(raw, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        if losses0 == "BCEWithLogitsLoss":
            return 1.0 / (1.0 + np.exp(-x))
        if losses0 in SOFTMAX:
            e = np.exp(x - np.max(x, axis=-1, keepdims=True))
            return e / np.sum(e, axis=-1, keepdims=True)
    return x


def transform_bound(raw, losses0):
    """relative bound (see the module docstring); 0 without a transform: the kept values are then copies"""
    v = transform64(raw, losses0)
    with np.errstate(all="ignore"):
        o = O.oracle_transform(np.asarray(raw, F32), losses0).astype(np.float64)
        ok = np.isfinite(v) & np.isfinite(o) & (np.abs(v) >= FLOOR)
        res = np.abs(o[ok] - v[ok]) / np.abs(v[ok])
    return 2.0 * float(res.max()) if res.size else 0.0


def tie_keys(raw, losses0):
    """int64 [R,128]: equal where the transformed values are equal in any deterministic fp32 kernel"""
    x = np.asarray(raw, F32) + F32(0.0)      # -0.0 -> +0.0: equal numbers
    if losses0 == "BCEWithLogitsLoss":
        x = np.where(x >= F32(SIGMOID_ONE), F32(np.inf), np.where(x <= F32(SIGMOID_ZERO), F32(-np.inf), x)).astype(F32)
    k = np.ascontiguousarray(x).view(np.int32).astype(np.int64)
    return np.where(np.isnan(x), (1 << 40) + np.arange(x.shape[-1], dtype=np.int64), k)      # a NaN equals nothing


def rows_of(off, cnt, key, w, n_max):
    """the compactor's flat (key, weight) arrays as [R, n_max] rows: bins (-1 padded), values (0 padded)"""
    cnt = np.asarray(cnt, np.int64)
    R = cnt.shape[0]
    slot = np.arange(n_max)[None, :] < np.clip(cnt, 0, n_max)[:, None]
    idx = np.asarray(off, np.int64)[:, None] + np.arange(n_max)[None, :]
    bins = np.full((R, n_max), -1, np.int64)
    vals = np.zeros((R, n_max), F32)
    bins[slot] = np.asarray(key)[idx[slot]] & 127
    vals[slot] = np.asarray(w)[idx[slot]]
    return bins, vals


def pack(K, vals32, n_max):
    """kept-set masks [R,128] + the fp32 transformed rows -> (cnt, bins, w) as O.select_adaptive returns them"""
    K = np.asarray(K, bool)
    cnt = K.sum(1).astype(np.int32)
    order = np.argsort(~K, axis=1, kind="stable")[:, :n_max]
    slot = np.arange(n_max)[None, :] < cnt[:, None]
    return cnt, np.where(slot, order, -1).astype(np.int16), np.where(slot, np.take_along_axis(np.asarray(vals32, F32), order, 1), F32(0)).astype(F32)


def kept_mask(cnt, bins):
    cnt = np.asarray(cnt, np.int64)
    bins = np.asarray(bins, np.int64)
    slot = np.arange(bins.shape[1])[None, :] < np.clip(cnt, 0, bins.shape[1])[:, None]
    K = np.zeros((cnt.shape[0], 128), bool)
    K[np.nonzero(slot)[0], np.clip(bins, 0, 127)[slot]] = True
    return K


def rule64(v, n_max, thr):
    """the set rule on fp64 values: the n_max largest (lower bin first among equals) that reach thr, else the arg-max alone; a NaN
    never ranks; an all-NaN row keeps bin 0.  -> kept mask, number of values that reach thr, rank order [R,128]"""
    nan = np.isnan(v)
    vc = np.where(nan, -np.inf, v)
    bin_ = np.broadcast_to(np.arange(v.shape[1]), v.shape)
    order = np.lexsort((bin_, nan, -vc), axis=-1)
    rank = np.argsort(order, axis=1)
    reach = (vc >= thr) & ~nan
    c = reach.sum(1)
    n_eff = np.where(c == 0, 1, n_max)
    return (rank < n_eff[:, None]) & (reach | (c == 0)[:, None]), c, order


def verdict(raw, losses0, n_max, thr, cnt, bins, w, bound):
    """-> dict(bad [R] bool, reasons {name: [R] bool}, decided [R] bool, worst relative residual of the kept values)"""
    raw = np.asarray(raw, F32)
    R = raw.shape[0]
    t = float(F32(thr))
    v = transform64(raw, losses0)
    nan, fin = np.isnan(v), np.isfinite(v)
    with np.errstate(all="ignore"):
        e = np.where(fin, bound * np.abs(v) + FLOOR, 0.0)
        lo, hi = v - e, v + e
    cnt = np.asarray(cnt, np.int64).reshape(R)
    bins = np.asarray(bins, np.int64).reshape(R, -1)[:, :n_max]
    w = np.asarray(w, F32).reshape(R, -1)[:, :n_max]
    if bins.shape[1] < n_max:      # callers may pass rows shorter than n_max when no count reaches it
        bins = np.pad(bins, ((0, 0), (0, n_max - bins.shape[1])), constant_values=-1)
        w = np.pad(w, ((0, 0), (0, n_max - w.shape[1])))
    why = {}
    slot = np.arange(n_max)[None, :] < np.clip(cnt, 0, n_max)[:, None]
    why["count outside 1..n_max"] = (cnt < 1) | (cnt > n_max)
    why["bin outside 0..127"] = (slot & ((bins < 0) | (bins > 127))).any(1)
    why["bins do not ascend"] = (slot[:, 1:] & (np.diff(bins, axis=1) <= 0)).any(1)
    bs = np.clip(bins, 0, 127)
    K = kept_mask(cnt, bins)
    allnan = nan.all(1)
    # kept values
    vk, ek = np.take_along_axis(v, bs, 1), np.take_along_axis(e, bs, 1)
    with np.errstate(all="ignore"):
        w64 = w.astype(np.float64)
        near = np.where(np.isinf(vk), w64 == vk, np.abs(w64 - vk) <= ek)
        rel = np.where(slot & np.isfinite(vk) & (np.abs(vk) >= FLOOR), np.abs(w64 - vk) / np.abs(vk), 0.0)
    why["kept value outside the bound"] = (slot & ~np.isnan(vk) & ~near).any(1)
    worst = float(np.nanmax(rel)) if rel.size else 0.0
    # NaN
    why["all-NaN row does not keep bin 0 alone"] = allnan & ~((cnt == 1) & (bins[:, 0] == 0) & np.isnan(w[:, 0]))
    why["kept bin with a NaN value"] = ~allnan & (K & nan).any(1)
    # eps-rule
    Kn, L = K & ~nan, ~K & ~nan
    with np.errstate(all="ignore"):
        kept_hi_min = np.where(Kn, hi, np.inf).min(1)
        kept_hi_max = np.where(Kn, hi, -np.inf).max(1)
        below = lo < t
        full = (cnt >= n_max)[:, None]
        regular = (kept_hi_min >= t) & (~L | below | (full & (lo <= kept_hi_min[:, None]))).all(1)
        fallback = (cnt == 1) & (kept_hi_max < t) & (nan | below).all(1) & (kept_hi_max >= np.where(nan, -np.inf, lo).max(1))
    why["neither a regular nor a fallback selection within the bound"] = ~allnan & ~(regular | fallback)
    # ties of equal inputs: in (key, bin) order no kept bin may follow a left-out bin of its own key
    key = tie_keys(raw, losses0)
    order = np.argsort(key, axis=1, kind="stable")
    ks, Ks = np.take_along_axis(key, order, 1), np.take_along_axis(K, order, 1)
    left = np.cumsum(~Ks, axis=1)
    start = np.concatenate([np.ones((R, 1), bool), ks[:, 1:] != ks[:, :-1]], 1)
    base = np.maximum.accumulate(np.where(start, left - ~Ks, 0), axis=1)
    why["tie resolved to the higher bin"] = ~allnan & (Ks & (left - base > 0) & (ks < (1 << 40))).any(1)
    # decided with margin -> the fp64 set rule, exactly
    vr = v
    if losses0 == "BCEWithLogitsLoss":      # the two saturated classes rank as the equal values they are in fp32
        vr = np.where(raw >= F32(SIGMOID_ONE), 1.0, np.where(raw <= F32(SIGMOID_ZERO), 0.0, v))
    expK, c, rank_order = rule64(vr, n_max, t)
    with np.errstate(all="ignore"):
        thr_margin = (nan | (np.abs(v - t) > 2 * e)).all(1)
        n_eff = np.where(c == 0, 1, n_max)
        need_cut = ((c == 0) | (c > n_max)) & (n_eff < 128)
        ia, ib = np.clip(n_eff - 1, 0, 127), np.clip(n_eff, 0, 127)
        a = np.take_along_axis(rank_order, ia[:, None], 1)[:, 0]
        b = np.take_along_axis(rank_order, ib[:, None], 1)[:, 0]
        rr = np.arange(R)
        b_nan = nan[rr, b]
        va, vb, ea, eb = v[rr, a], v[rr, b], e[rr, a], e[rr, b]
        gap_ok = (va - vb) > 2 * np.maximum(ea, eb)
        tied = key[rr, a] == key[rr, b]
        others = ~nan & (key != key[rr, a][:, None])
        tie_ok = (~others | (np.abs(v - va[:, None]) > 2 * np.maximum(e, ea[:, None]))).all(1)
        cut_ok = ~need_cut | b_nan | np.where(tied, tie_ok, gap_ok)
    decided = allnan | (thr_margin & cut_ok)
    why["decided with margin, but not the fp64 rule's set"] = decided & (K != expK).any(1)
    bad = np.zeros(R, bool)
    for m in why.values():
        bad |= m
    return dict(bad=bad, reasons=why, decided=decided, worst=worst, expected=expK)


def check_selection(raw, losses0, n_max, thr, cnt, bins, w, bound, log=None):
    """asserts that no ray is bad; -> dict(rays, undecided, worst, bound, decided)"""
    r = verdict(raw, losses0, n_max, thr, cnt, bins, w, bound)
    out = dict(rays=int(r["bad"].size), undecided=int((~r["decided"]).sum()), worst_residual=r["worst"], bound=float(bound))
    if log:
        log(dict(out, n_max=int(n_max), thr=float(thr), bad=int(r["bad"].sum())))
    if r["bad"].any():
        lines = ["%s: rays %s" % (k, np.flatnonzero(m)[:8].tolist()) for k, m in r["reasons"].items() if m.any()]
        raise AssertionError("%s n_max %d thr %r: %d of %d rays are wrong\n  %s" % (losses0, n_max, thr, int(r["bad"].sum()), r["bad"].size, "\n  ".join(lines)))
    out["decided"] = r["decided"]
    return out


# ---- fp32 restatements of the two softmax summation orders ----------------------------------------------------------------------------

def transform32_pair(raw, losses0):
    """O.oracle_transform with the softmax sum in pair_epilogue's order: two serial sums of 64 values (the halves (bin // 4) % 2, bins
    ascending), then added"""
    raw = np.asarray(raw, F32)
    if losses0 not in SOFTMAX:
        return O.oracle_transform(raw, losses0)
    with np.errstate(all="ignore"):
        ex = np.exp(raw - np.max(raw, axis=-1, keepdims=True), dtype=F32)
        half = (np.arange(128) // 4) % 2
        s = []
        for h in (0, 1):
            acc = np.zeros(raw.shape[0], F32)
            for i in np.flatnonzero(half == h):
                acc = (acc + ex[:, i]).astype(F32)
            s.append(acc)
        return (ex / (s[0] + s[1]).astype(F32)[:, None]).astype(F32)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------

def _first(bins):
    return lambda n_max, thr: list(bins)[:n_max]


def edge_rows(losses0):
    """[(name, row [128] fp32, expect(n_max, thr) -> kept bins)] for thr in THRESHOLDS[losses0] and BOUNDARY"""
    f = lambda fill: np.full(128, fill, F32)
    out = []
    if losses0 == "BCEWithLogitsLoss":
        x = f(-5.0)      # sigmoid(-5) = 0.0067: below every threshold in use
        x[10:30] = np.arange(30, 50)      # twenty distinct logits, all exactly 1.0f: a tie, so the lowest bins and not the largest logits
        out.append(("saturated", x, _first(range(10, 30))))
        out.append(("all -200: exactly 0", f(-200.0), _first([0])))
        x = f(-5.0)
        x[5], x[70] = 0.0, -0.0      # both exactly 0.5: kept by >= at 0.5 and below, equal arg-maxima above
        out.append(("logit 0 and -0", x, lambda n_max, thr: [5, 70][:n_max] if thr <= 0.5 else [5]))
        x = f(-5.0)
        x[[3, 100]], x[[0, 50]] = np.inf, -np.inf
        out.append(("+inf and -inf", x, _first([3, 100])))
        out.append(("all -inf: exactly 0", f(-np.inf), _first([0])))
        x = f(-5.0)
        x[[0, 64]], x[7] = np.nan, 3.0
        out.append(("NaN among numbers", x, _first([7])))
        out.append(("all NaN", f(np.nan), _first([0])))
    elif losses0 in SOFTMAX:
        for c in (0.0, 2.5, -7.0):      # 128 x expf(0) = 128 in any order: every value exactly 1/128
            out.append(("all equal %g" % c, f(c), lambda n_max, thr: list(range(n_max)) if thr <= 1.0 / 128.0 else [0]))
        x = f(0.0)
        x[37] = 100.0
        out.append(("one-hot", x, _first([37])))
        x = f(-np.inf)
        x[[20, 90]] = 1.5      # each exactly 0.5
        out.append(("two maxima, -inf elsewhere", x, _first([20, 90])))
        x = np.random.default_rng(5).uniform(-2, 2, 128).astype(F32)
        x[9] = np.inf
        out.append(("+inf: all NaN", x, _first([0])))
        out.append(("all -inf: all NaN", f(-np.inf), _first([0])))
        x = np.random.default_rng(6).uniform(-2, 2, 128).astype(F32)
        x[101] = np.nan
        out.append(("one NaN: all NaN", x, _first([0])))
    else:      # the edge rows of test_gpu_parity.test_compact_edge_cases_bit_exact
        out.append(("all 0.5", f(0.5), _first(range(128))))
        out.append(("all -1", f(-1.0), _first([0])))
        x = f(0.0)
        x[[3, 5, 70, 90, 100]] = 0.7
        out.append(("five-way tie", x, _first([3, 5, 70, 90, 100])))
        x = f(0.0)
        x[127] = 1.0
        out.append(("last bin", x, _first([127])))
        out.append(("all NaN", f(np.nan), _first([0])))
        x = f(np.nan)
        x[77] = -3.0
        out.append(("one number", x, _first([77])))
        x = f(-1.0)
        x[10:30] = np.inf
        out.append(("twenty +inf", x, _first(range(10, 30))))
        out.append(("all -inf", f(-np.inf), _first([0])))
        x = f(-1.0)
        x[[0, 127]] = 0.9
        out.append(("first and last bin", x, _first([0, 127])))
        x = f(-1.0)
        x[64], x[3] = np.nan, 0.75
        out.append(("NaN among numbers", x, _first([3])))
        x = f(-1.0)      # one +inf above twenty distinct candidates (ascending with the bin): +inf first, then the LARGEST of the others
        x[40] = np.inf
        x[50:70] = np.linspace(0.6, 2.5, 20)
        out.append(("+inf above candidates", x, lambda n_max, thr: [40] + list(range(71 - min(n_max, 21), 70))))
    return out


def selection_inputs(seed, losses0, n_random=640, n_quant=320):
    """-> dict(raw [R,128] fp32, kind [R] ('random' | 'quantised' | 'large' | 'edge'), edges [(row index, name, expect)])"""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.3, 3.0, (n_random, 1))
    offset = rng.uniform(-3.0, 1.0, (n_random, 1))
    rnd = (rng.standard_normal((n_random, 128)) * scale + offset).astype(F32)
    p = rng.dirichlet(np.full(6, 0.6), n_quant)      # own level frequencies per row: the cut-off falls into every level
    u = rng.uniform(0, 1, (n_quant, 128, 1))
    q = LEVELS[(u > np.cumsum(p, 1)[:, None, :]).sum(2).clip(0, 5)]
    rows, kind = [rnd, q], ["random"] * n_random + ["quantised"] * n_quant
    if losses0 in SOFTMAX:      # logits near 1e4 (spacing 2^-10): only a softmax that subtracts the maximum survives
        big = (1.0e4 + rng.uniform(-3, 3, (16, 128))).astype(F32)
        rows.append(big)
        kind += ["large"] * 16
    edges = edge_rows(losses0)
    first = len(kind)
    rows.append(np.stack([x for _, x, _ in edges]))
    kind += ["edge"] * len(edges)
    return dict(raw=np.ascontiguousarray(np.concatenate(rows), F32), kind=np.array(kind),
                edges=[(first + i, name, expect) for i, (name, _, expect) in enumerate(edges)])


def thresholds(losses0):
    return (THRESHOLDS[losses0],) + BOUNDARY


def assert_edges(inputs, n_max, thr, cnt, bins, what=""):
    for row, name, expect in inputs["edges"]:
        got = [int(b) for b in np.asarray(bins)[row, :int(cnt[row])]]
        want = expect(n_max, float(F32(thr)))
        assert got == want, "%s edge row %r at n_max %d thr %r: kept bins %s, expected %s" % (what, name, n_max, thr, got, want)


# ---- the guarded two-precision selection (ADANERF_SAMPLING_GUARDED) under every transform ------------------------------------------------
#
# adanerf_compact_guarded selects from `approx` with a guard band, re-selects the rays the band leaves undecided from `exact`, and owes
# the selection of `exact` bit for bit whenever |approx - exact| <= eps on every raw value.  The band in transformed units
# (k_select_pair.hip.hpp guard_band_of / pair_select): e = eps (none), eps / 4 (sigmoid), 1.01 (exp(2 eps) - 1) max(p~) (softmax); pair
# bound 2 e.  With c the ray's values sorted descending and n = n_max the rule reads (restated independently of
# adanerf_oracle.guard_undecided, which test_guarded_transforms_cpu holds it against):
#   undecided  <=>  a raw value is not finite,
#               or  |c_k - thr| <= e for a k < n,
#               or  c_0 >= thr and c_n >= max(c_{n-1} - 2 e, thr - e)        (a runner-up within the pair bound of the cut, or a tie)
#               or  c_0 <  thr and c_1 >= c_0 - 2 e                          (the arg-max fallback)
#
#   guard_classes    the rule in float64 on transform64(approx), evaluated twice: `must` = undecided however a correct fp32 kernel rounds,
#                    `may` = undecided for some correct fp32 kernel.  What a correct kernel may differ by, per ray:
#                      rho    on every transformed value and hence (order statistics are 1-Lipschitz) on every c_k:
#                             transform_bound(approx) * max(v) + FLOOR, the bound check_selection holds the kept values to
#                      slack  on each side of a comparison, for the fp32 subtractions c_k - thr, c_{n-1} - 2 e, thr - e: 2^-22 max(c_0, thr)
#                      beta   relative, on the softmax factor 1.01f (expf(2 eps) - 1): an expf within 2 ulp of 1 (2^-22 absolute) loses
#                             2^-22 / (exp(2 eps) - 1) relative in the subtraction, plus two roundings (2^-22)
#                    Without a transform nothing is rounded differently -- the kernel's expressions are single IEEE operations numpy
#                    repeats -- so the rule is evaluated in fp32 and must == may.
#   guard_inputs     exact = the base rows of selection_inputs + band rows; approx = fp32(exact + s dmax), |s| <= 1,
#                    dmax = max(0, min(0.999 eps, eps - 64 spacing(|exact|))) (the reserve keeps the fp32 rounding of approx and of
#                    the kernel's differences far below the slack; it removes the perturbation from the logits near 1e4).
#                    Band rows are built as the APPROXIMATE row in transformed space -- the critical quantity (a value's distance from thr in
#                    units of e, or the gap between the n-th and the (n+1)-th value in units of 2 e) at GUARD_PLACES -- mapped back
#                    (logit / log p + a constant) and moved by 0.999 eps against the adversarial direction of their kind to give the
#                    exact row, so that kind's perturbation lands them on the placement.  They sit where the band is nearly tight:
#                    sigmoid values near 0.5; softmax rows whose largest bin is thr + 2.5 e, the critical bin beside it, and the other
#                    97 % of the mass in 126 bins a dozen bands below thr, so that max(p~) is within a few per cent of the critical value.
#                    What cannot have teeth, and why: a threshold row whose critical value is the ray's only candidate (n_max = 1) keeps
#                    the arg-max on either side of thr; a softmax gap row never flips below the kernel's pair bound, because the ratio of
#                    two probabilities of one row moves by exp(2 eps) at most while 2 e allows each of them that much (the pair bound is
#                    conservative by 2 there).  So under the softmax with n_max = 1 no row can be selected wrongly by a band of 0.5 or
#                    0.8 eps: test_guarded_transforms_cpu asserts exactly that instead of teeth.
#   check_guarded    what a device result (or an emulated faulty one) owes: see its docstring.

GUARD_PLACES = (0.55, 0.7, 0.9, 1.1, 1.5)
GUARD_PUSH = 0.999
GUARD_EPS = (0.01, 0.002)
GUARD_N = (1, 2, 4, 5, 8, 9, 16)
TRANSFORM_NAME = {"MSE": "none", "BCEWithLogitsLoss": "sigmoid", "CrossEntropyLoss": "softmax", "CrossEntropyLossWeighted": "softmax"}


def guard_thresholds(losses0):
    return (THRESHOLDS[losses0],) + (() if losses0 in SOFTMAX else (0.5,))


def rule32(y32, n_max, thr, e, ep=None):
    """the rule in fp32 on transformed fp32 rows with a caller-chosen band e [R] (and pair bound): what a kernel with another band computes"""
    y = np.asarray(y32, F32)
    bad = ~np.isfinite(y).all(1)
    s = -np.sort(-np.where(bad[:, None], F32(0), y), axis=1)
    return _guard_rule(s, n_max, F32(thr), np.asarray(e, F32), 0, 0, 1, None if ep is None else np.asarray(ep, F32)) | bad


def guard_factor(losses0, eps):
    """guard_band_of in float64 on the fp32 eps the kernel receives: the band in transformed units (softmax: per unit of max(p~))"""
    eps = float(F32(eps))
    if losses0 == "BCEWithLogitsLoss":
        return 0.25 * eps
    if losses0 in SOFTMAX:
        return float(F32(1.01)) * float(np.expm1(2.0 * eps))
    return eps


def _guard_rule(s, n, t, e, rho, slack, sign, ep=None):
    """the rule on descending rows s [R,128]; sign = +1 widens every comparison by (rho, slack), -1 narrows it.  fp32 in, fp32 arithmetic.
    ep: a pair bound other than 2 e (the kernel never uses one under a transform; the faulty kernels of the rejection test do)"""
    w = sign * rho
    ep = 2 * e if ep is None else ep
    a = (np.abs(s[:, :n] - t) <= (e + w + sign * slack)[:, None]).any(1)
    reg = s[:, n] + w >= np.maximum(s[:, n - 1] - w - ep, t - e) - sign * slack
    fb = s[:, 1] + w >= s[:, 0] - w - ep - sign * slack
    return a | np.where(s[:, 0] < t, fb, reg)


def guard_classes(approx, losses0, n_max, thr, eps):
    """-> must, may (bool [R]); rays in may & ~must are borderline"""
    approx = np.asarray(approx, F32)
    R = approx.shape[0]
    bad = ~np.isfinite(approx).all(1)
    x = np.where(bad[:, None], F32(0), approx)      # their class is settled; keep them out of the arithmetic
    if TRANSFORM_NAME.get(losses0, "none") == "none":
        s = -np.sort(-x, axis=1)
        und = _guard_rule(s, n_max, F32(thr), np.full(R, F32(eps), F32), 0, 0, 1) | bad
        return und, und.copy()
    t = float(F32(thr))
    s = -np.sort(-transform64(x, losses0), axis=1)
    rho = transform_bound(x, losses0) * s[:, 0] + FLOOR
    slack = 2.0 ** -22 * np.maximum(s[:, 0], t)
    f = guard_factor(losses0, eps)
    if losses0 in SOFTMAX:
        beta = 2.0 ** -22 / float(np.expm1(2.0 * float(F32(eps)))) + 2.0 ** -22
        e_lo, e_hi = f * (1 - beta) * (s[:, 0] - rho), f * (1 + beta) * (s[:, 0] + rho)
    else:
        e_lo = e_hi = np.full(R, f)
    return _guard_rule(s, n_max, t, e_lo, rho, slack, -1) | bad, _guard_rule(s, n_max, t, e_hi, rho, slack, 1) | bad


def _inverse(losses0, y, const=0.0):
    if losses0 == "BCEWithLogitsLoss":
        return np.log(y / (1.0 - y))
    if losses0 in SOFTMAX:
        return np.log(y) + const
    return y


def _band_rows(rng, losses0, n_max, thr, eps):
    """-> exact rows [B,128] float64 (raw), meta [(type 'thr' | 'cut', place, critical bin, direction of the critical bin under the row's kind)]
    Each row is laid out as the approximate row (y / p: transformed values, the critical quantity at place m; side: above / below thr), then
    exact = approx - s push, s = the direction the row's own kind (thr / one for 'thr' rows, cut for 'cut' rows) gives every entry of
    that exact row: for m < 1 the exact value lies across thr (the exact order across the cut) and the selection flips where the band is tight,
    for m > 1 it lies further out on the same side (softmax gap rows keep their order for every m: they cannot flip)."""
    f = guard_factor(losses0, eps)
    push = GUARD_PUSH * float(F32(eps))
    soft, sig = losses0 in SOFTMAX, losses0 == "BCEWithLogitsLoss"
    if n_max == 1:      # a threshold row teaches nothing there
        reps = {"cut": 11}
    elif soft:          # a gap row has no teeth there
        reps = {"thr": 9, "cut": 3}
    else:
        reps = {"thr": 6, "cut": 6}
    rows, meta = [], []
    for typ, n_rep in reps.items():
        for m in GUARD_PLACES:
            for side in (1, -1):
                for _ in range(n_rep):
                    bins = rng.permutation(128)
                    s = np.zeros(128)
                    if soft:
                        const = 4.6 + rng.uniform(-0.3, 0.3)
                        if typ == "thr":
                            top = thr * (1.0 + rng.uniform(0, 0.02)) / (1.0 - 2.5 * f)
                            c = bins[1]
                            p = np.zeros(128)
                            p[bins[0]], p[c] = top, thr + side * m * f * top
                            bg = rng.uniform(0.85, 1.15, 126)
                            p[bins[2:]] = (1.0 - p.sum()) * bg / bg.sum()
                            s[:] = -(side if m < 1 else -side)
                            s[c] = -s[c]
                        else:
                            v = min(0.03, 0.4 / n_max)
                            p = np.zeros(128)
                            p[bins[:n_max - 1]] = v * rng.uniform(1.02, 1.12, n_max - 1)
                            c = bins[n_max - 1]
                            p[c] = v
                            p[bins[n_max]] = v - m * 2 * f * p.max()
                            bg = rng.uniform(0.85, 1.15, 127 - n_max)
                            p[bins[n_max + 1:]] = (1.0 - p.sum()) * bg / bg.sum()
                            s[:] = 1
                            s[bins[:n_max]] = -1
                        x = _inverse(losses0, p, const) - s * push
                    else:
                        e = f
                        hi = 0.97 if sig else thr + 0.6
                        y = rng.uniform(0.02, thr - 0.15, 128) if sig else rng.uniform(thr - 0.8, thr - 0.3, 128)
                        if typ == "thr":
                            k = int(rng.integers(1, min(n_max - 1, 4) + 1))
                            y[bins[:k]] = rng.uniform(thr + 8 * e + 0.02, hi, k)
                            c = bins[k]
                            y[c] = thr + side * m * e
                            s[c] = side if m < 1 else -side
                        else:
                            below = n_max == 1 and side < 0      # the arg-max fallback's runner-up
                            v = thr + (-1 if below else 1) * rng.uniform(6, 8) * e
                            y[bins[:n_max - 1]] = rng.uniform(v + 8 * e, hi, n_max - 1)
                            c, b = bins[n_max - 1], bins[n_max]
                            y[c], y[b] = v, v - m * 2 * e
                            s[c], s[b] = (1, -1) if m < 1 else (-1, 1)
                        x = _inverse(losses0, y) - s * push
                    rows.append(x)
                    meta.append((typ, m, int(c), int(s[c])))
    return np.stack(rows), meta


def _perturbations(rng, exact, losses0, n_max, thr, first_band, meta):
    """[(kind, s [R,128] in [-1, 1])]: directions in raw space, from the exact rows alone (and, for `one`, the band rows' critical bins)"""
    R = exact.shape[0]
    fin = np.isfinite(exact)
    with np.errstate(all="ignore"):
        v = transform64(exact, losses0)
    out = [("rand", rng.uniform(-1, 1, exact.shape))]
    out.append(("thr", np.nan_to_num(np.sign(float(F32(thr)) - v), nan=0.0, posinf=0.0, neginf=0.0)))
    rank = np.argsort(np.argsort(-np.where(fin, exact, -np.inf).astype(np.float64), axis=1, kind="stable"), axis=1)
    out.append(("cut", np.where(rank < n_max, -1.0, 1.0)))
    if losses0 in SOFTMAX:      # one bin against all the others
        with np.errstate(all="ignore"):
            d = np.abs(np.log(v / float(F32(thr))))
        c = np.argmin(np.where(np.isfinite(d), d, np.inf), axis=1)
        vc = v[np.arange(R), c]
        sc = np.where(vc < float(F32(thr)), 1.0, -1.0)
        for i, (typ, m, cb, scb) in enumerate(meta):
            if typ == "thr":
                c[first_band + i], sc[first_band + i] = cb, scb
        s = -np.repeat(sc[:, None], 128, 1)
        s[np.arange(R), c] = sc
        out.append(("one", s))
    return out


def guard_inputs(seed, losses0, n_max, thr, eps):
    """-> dict(exact [R,128] fp32, approx [(kind, [R,128] fp32)], first_band, meta (see _band_rows),
              expect [(kind, rows, 'must' | 'outside')]: the class the band rows were built to have under the kind they were built for)"""
    eps32 = float(F32(eps))
    base = selection_inputs(seed, losses0)["raw"]
    rng = np.random.default_rng([seed, n_max, int(round(thr * 1e6)), int(round(eps * 1e6)), LOSSES.index(losses0) if losses0 in LOSSES else 3])
    band, meta = _band_rows(rng, losses0, n_max, thr, eps)
    exact = np.ascontiguousarray(np.concatenate([base, band.astype(F32)]), F32)
    first = base.shape[0]
    fin = np.isfinite(exact)
    x64 = np.where(fin, exact, 0).astype(np.float64)
    dmax = np.maximum(0.0, np.minimum(GUARD_PUSH * eps32, eps32 - 64.0 * np.spacing(np.abs(x64).astype(F32)).astype(np.float64)))
    approx = []
    for kind, s in _perturbations(rng, exact, losses0, n_max, thr, first, meta):
        assert (np.abs(s) <= 1).all()
        a = np.where(fin, (x64 + s * dmax).astype(F32), exact).astype(F32)
        assert (np.abs(a.astype(np.float64)[fin] - x64[fin]) <= eps32).all(), "input condition: |approx - exact| <= eps"
        assert same_nonfinite(a, exact)
        approx.append((kind, np.ascontiguousarray(a)))
    typ = np.array([m[0] for m in meta])
    place = np.array([m[1] for m in meta])
    own = {"thr": "one" if losses0 in SOFTMAX else "thr", "cut": "cut"}
    expect = []
    for t in np.unique(typ):
        expect.append((own[t], first + np.flatnonzero((typ == t) & (place < 1)), "must"))
        expect.append((own[t], first + np.flatnonzero((typ == t) & (place > 1)), "outside"))
    return dict(exact=exact, approx=approx, first_band=first, meta=meta, expect=expect)


def same_nonfinite(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nf = ~np.isfinite(b)
    return bool((np.isfinite(a) == np.isfinite(b)).all() and np.array_equal(a.view(np.uint32)[nf], b.view(np.uint32)[nf]))


def assert_guard_conditions(must, may, what):
    """the input condition of a (case, kind): few borderline rays, both classes well populated -> (borderline, outside, inside)"""
    R = must.size
    assert not (must & ~may).any(), what + ": must is not inside may"
    border, outside, inside = int((may & ~must).sum()), int((~may).sum()), int(must.sum())
    assert border <= 0.01 * R, "%s: %d of %d rays are borderline" % (what, border, R)
    assert outside >= 0.05 * R and inside >= 0.05 * R, "%s: %d rays outside may, %d inside must, of %d" % (what, outside, inside, R)
    return border, outside, inside


def selection_of(rows32, n_max, thr):
    """what adanerf_compact owes on transformed fp32 rows, as the dict the GPU tests build: cnt, off, total, key, bins, vals"""
    with np.errstate(all="ignore"):
        cnt, bins, vals = O.select_adaptive(np.asarray(rows32, F32), n_max, thr)
    off, ray, b, w = O.compact(cnt, bins, vals)
    return dict(cnt=cnt, off=off, total=int(cnt.sum()), key=((ray.astype(np.uint32) << 7) | b.astype(np.uint32)), bins=bins.astype(np.int64), vals=vals)


def row_max_diff(approx, exact, rows):
    """the monitor's statistic over `rows`: the largest finite fp32 |approx - exact|, 0 where there is none"""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(approx, F32)[rows] - np.asarray(exact, F32)[rows])
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def check_guarded(losses0, approx, exact, must, may, G, CX, CY, exact_refined=None):
    """G: a result of adanerf_compact_guarded(approx, exact) -- dict(cnt, off, total, key, bins [R,n], vals [R,n], refined, and with a monitor
    mon = dict(max_diff, violations, max_pair, audit_mismatch, audited)); CX / CY: adanerf_compact(exact) / (approx) in the same context.
      a. the selection is CX's: counts, offsets, total and keys, bit for bit
      b. the kept values of a ray are CX's row or CY's row, bit for bit and never a mixture; CX's on every ray in `must` (which holds every
         row with a NaN or an infinity), CY's on every ray outside `may`
      c. must.sum() <= refined <= may.sum(); exact_refined (no transform: the fp32 rule's count) is met exactly
      d. (no audit) no violation, max_diff between the row maxima of |approx - exact| over must and over may, no pair statistic under a
         transform, nothing audited
    -> dict(refined, borderline, carried_exact: rays whose row is CX's and not CY's)"""
    R = must.size
    for k in ("cnt", "off", "key"):
        assert np.array_equal(np.asarray(G[k]), np.asarray(CX[k])), "guarded %s differ from the exact selection's" % k
    assert int(G["total"]) == int(CX["total"]), "guarded total differs from the exact selection's"
    assert np.array_equal(G["bins"], CX["bins"]), "guarded bins differ from the exact selection's"
    is_x = (_bits(G["vals"]) == _bits(CX["vals"])).all(1)
    is_y = (_bits(G["vals"]) == _bits(CY["vals"])).all(1) & (np.asarray(CY["cnt"]) == np.asarray(G["cnt"])) & (CY["bins"] == G["bins"]).all(1)
    assert (is_x | is_y).all(), "rays %s carry neither the exact nor the approximate row" % np.flatnonzero(~(is_x | is_y))[:8].tolist()
    assert is_x[must].all(), "undecided rays %s do not carry the exact row" % np.flatnonzero(must & ~is_x)[:8].tolist()
    assert is_y[~may].all(), "decided rays %s do not carry the approximate row" % np.flatnonzero(~may & ~is_y)[:8].tolist()
    assert must[~np.isfinite(np.asarray(approx, F32)).all(1)].all()
    lo, hi, refined = int(must.sum()), int(may.sum()), int(G["refined"])
    assert lo <= refined <= hi, "refined %d outside [%d, %d]" % (refined, lo, hi)
    assert exact_refined is None or refined == int(exact_refined), "refined %d, the rule gives %d" % (refined, int(exact_refined))
    if "mon" in G:
        mon = G["mon"]
        assert mon["violations"] == 0, "the monitor reports %d violations of a band that holds" % mon["violations"]
        d_lo, d_hi = row_max_diff(approx, exact, must), row_max_diff(approx, exact, may)
        assert d_lo <= mon["max_diff"] <= d_hi, "monitor max_diff %r outside [%r, %r]" % (mon["max_diff"], d_lo, d_hi)
        assert TRANSFORM_NAME.get(losses0, "none") == "none" or mon["max_pair"] == 0.0, "a pair statistic under a transform"
        assert mon["audited"] == 0 and mon["audit_mismatch"] == 0, "audit counters without an audit"
    return dict(refined=refined, borderline=hi - lo, carried_exact=int((is_x & ~is_y).sum()))


def emulate_guarded(losses0, approx, exact, n_max, thr, eps, undecided=None, fault=None):
    """a guarded result built on the CPU from the fp32 numpy restatements; `undecided` replaces the rule's verdict (a faulty band),
    fault: 'refined keeps approx' | 'decided carries exact' | 'refined + 1' -> G, CX, CY as check_guarded takes them"""
    approx, exact = np.asarray(approx, F32), np.asarray(exact, F32)
    with np.errstate(all="ignore"):
        ya, yx = O.oracle_transform(approx, losses0), O.oracle_transform(exact, losses0)
        if undecided is None:
            undecided = O.guard_undecided(ya, n_max, thr, eps, TRANSFORM_NAME.get(losses0, "none"))
    und = np.asarray(undecided, bool) | ~np.isfinite(approx).all(1)
    CX, CY = selection_of(yx, n_max, thr), selection_of(ya, n_max, thr)
    cnt = np.where(und, CX["cnt"], CY["cnt"])
    bins = np.where(und[:, None], CX["bins"], CY["bins"])
    from_x = np.ones_like(und) if fault == "decided carries exact" else (np.zeros_like(und) if fault == "refined keeps approx" else und)
    vals = np.where(bins >= 0, np.take_along_axis(np.where(from_x[:, None], yx, ya), np.clip(bins, 0, 127), 1), F32(0)).astype(F32)
    off, ray, b, w = O.compact(cnt, bins, vals)
    G = dict(cnt=cnt, off=off, total=int(cnt.sum()), key=(ray.astype(np.uint32) << 7) | b.astype(np.uint32), bins=bins, vals=vals)
    G["refined"] = int(und.sum()) + (1 if fault == "refined + 1" else 0)
    pairs = TRANSFORM_NAME.get(losses0, "none") == "none"
    with np.errstate(all="ignore"):
        pe = O.guard_pair_error(approx, exact, n_max, thr, eps)[und & np.isfinite(approx).all(1)] if pairs else np.zeros(0, F32)
    G["mon"] = dict(max_diff=row_max_diff(approx, exact, und), violations=0, audited=0, audit_mismatch=0, max_pair=float(pe.max(initial=0)))
    return G, CX, CY
