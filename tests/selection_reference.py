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
