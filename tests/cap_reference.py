"""numpy restatement of the sample cap (adanerf_set_sample_cap / adanerf_compact_cap), by brute force: T is evaluated at every value present
in the batch, the smallest one that fits is t*, and the rows are trimmed at (N, t*) with the row trim of tests/budget_reference.py.  Exact
arithmetic only (integers and float comparisons), so everything that compares against this file compares bytes.  Also the rows built for
the places the device's selection of t* can go wrong; tests/test_cap_reference_cpu.py shows that they tell wrong rules from the right one.
Test infrastructure: nothing under adanerf_amd/ imports it."""
import numpy as np

import adanerf_oracle as O
import budget_reference as B

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)


def kept_total(count, wts, t):
    """T(t) = sum_r kept_r(t): 0 for an empty row, else max(1, #{k < c_r : v_rk >= t}) (a NaN never passes, -0 equals +0)"""
    count = np.asarray(count).astype(np.int64)
    live = np.arange(wts.shape[1])[None, :] < count[:, None]
    with np.errstate(invalid="ignore"):
        a = ((wts >= F32(t)) & live).sum(axis=1)
    return int(np.where(count == 0, 0, np.maximum(1, a)).sum())


def present_values(count, wts):
    """the non-NaN values of the live entries, -0 taken as +0, ascending, each once"""
    live = np.arange(wts.shape[1])[None, :] < np.asarray(count).astype(np.int64)[:, None]
    v = wts[live]
    v = v[~np.isnan(v)]
    v = np.where(v == 0, F32(0), v).astype(F32)
    return np.unique(v)


def threshold(count, wts, cap_total):
    """t* of a selection in select_adaptive's layout ([R] counts, [R, N] values) under C = cap_total: None if T_now <= C; else the
    smallest present value with T <= C, +inf if there is none"""
    if int(np.asarray(count).astype(np.int64).sum()) <= cap_total:
        return None
    fits = [v for v in present_values(count, wts) if kept_total(count, wts, v) <= cap_total]      # T at EVERY present value
    return F32(min(fits)) if fits else INF


def apply(count, bins, wts, cap_total):
    """(t* -- -inf if nothing is trimmed --, counts, bins, values) of the capped selection, select_adaptive's layout"""
    t = threshold(count, wts, cap_total)
    if t is None:
        return -INF, np.asarray(count).astype(np.int32), bins, wts
    R, n_max = wts.shape
    c, b, w = B.trim(count, bins, wts, np.full(R, n_max, np.int32), np.full(R, t, F32))
    return t, c, b, w


# ---- rows built for the places the device's selection can go wrong ---------------------------------------------------------------------
# A case is (oracle rows [n, 128] float32, n_max, thr, C): the selection at (n_max, thr) of those rows is what the cap sees.  Values are
# placed at bins 5 k + 3 in front of a fill below every threshold, so every kept value is chosen here.

FILL = F32(-2.0)
THR = 0.25


def rows_of(values, fill=FILL):
    """oracle rows from per-row lists of values (at most 25 each)"""
    orc = np.full((len(values), 128), fill, F32)
    for r, vs in enumerate(values):
        orc[r, 3:3 + 5 * len(vs):5] = np.asarray(vs, F32)
    return orc


def from_bits(bits):
    return np.asarray(bits, np.uint32).view(F32)


def selection(orc, n_max, thr):
    c, b, w = O.select_adaptive(orc, n_max, F32(thr))
    return c.astype(np.int32), b, w


def built_cases():
    """{name: (orc, n_max, thr, C)}; deterministic"""
    rng = np.random.default_rng(2024)
    out = {}
    n = 600
    # a tie at t* shared by hundreds of rows: T(0.3) = 4 n, T(0.5) = 3 n, T(0.9) = n, and C lies between 3 n and n
    out["tie_jump"] = (rows_of([[0.9, 0.5, 0.5, 0.3]] * n), 8, THR, 2 * n + n // 2)
    # the same tie with C exactly on T(0.5): the tie fits whole
    out["tie_fits"] = (rows_of([[0.9, 0.5, 0.5, 0.3]] * n), 8, THR, 3 * n)
    # all entries of the batch equal: no present value fits, t* = +inf, every row falls to its first entry
    out["all_equal"] = (rows_of([[0.5] * 8] * 300), 8, THR, 4 * 300)
    # values that differ only in their lowest 10 key bits / only in the middle 11: one radix level each decides
    lo = from_bits(0x3F000000 + rng.integers(0, 1024, (257, 8)))
    out["low10"] = (rows_of(lo), 8, THR, int(0.6 * 257 * 8))
    mid = from_bits(0x3F000000 + (rng.integers(0, 2048, (257, 8)) << 10))
    out["mid11"] = (rows_of(mid), 8, THR, int(0.6 * 257 * 8))
    top = from_bits((rng.integers(0x3E8, 0x3F8, (257, 8)) << 20))      # and only in the top bits
    out["top11"] = (rows_of(top), 8, THR, int(0.6 * 257 * 8))
    # fallback rows (one value below thr: negative, -0, +0, small) next to rows of positive values; a fallback value is never t*
    vals = []
    for r in range(400):
        k = r % 8
        if k == 0:
            vals.append([-0.8])
        elif k == 1:
            vals.append([-0.0])
        elif k == 2:
            vals.append([0.0])
        elif k == 3:
            vals.append([0.1, -0.5, -0.0])      # the arg-max alone
        else:
            vals.append(list(rng.choice(np.arange(0.25, 1.0, 1 / 64), 6).astype(F32)))
    fb = rows_of(vals)
    c_fb = selection(fb, 8, THR)[0]
    out["fallback_rows"] = (fb, 8, THR, int(c_fb.sum()) - 350)
    # +inf entries (one per row at most), next to finite ones; C so low that t* = +inf is a present value
    vals = [[np.inf, 0.6, 0.4] if r % 3 == 0 else [0.7, 0.7, 0.3] for r in range(300)]      # T(0.7) = 500, T(+inf) = 300
    out["inf_present"] = (rows_of(vals), 8, THR, 300)
    out["inf_above"] = (rows_of(vals), 8, THR, 500)
    # NaN rows: the selection keeps one NaN entry (the fallback of a row without a number); it counts 1 at every t
    nanrows = rows_of([[0.9, 0.6, 0.4, 0.3]] * 200)
    nanrows[::4] = NAN
    out["nan_fallback"] = (nanrows, 8, THR, 500)
    # the bounds themselves, on random rows with ties (multiples of 1 / 32)
    q = (np.round(rng.uniform(-0.5, 1.5, (257, 128)) * 32) / 32).astype(F32)
    tq = int(selection(q, 8, THR)[0].sum())
    out["c_is_n"] = (q, 8, THR, 257)                  # every row falls to one entry
    out["c_is_t_now"] = (q, 8, THR, tq)               # nothing is trimmed
    out["c_is_t_now_minus_1"] = (q, 8, THR, tq - 1)   # the least trim there is
    out["c_above_t_now"] = (q, 8, THR, tq + 1000)
    # long rows (a wave per ray on the device), ties included
    q24 = (np.round(rng.uniform(-0.5, 1.5, (257, 128)) * 64) / 64).astype(F32)
    out["long_rows"] = (q24, 24, THR, int(0.7 * selection(q24, 24, THR)[0].sum()))
    return out


def random_case(n, n_max, seed=0):
    """(orc, n_max, thr, C) for a batch of n rays: about 8 of a row's 128 values reach the threshold, so counts run from the arg-max
    fallback to n_max; continuous values for small batches, multiples of 2^-12 above (the brute-force reference evaluates T at every
    present value); C = 0.7 T_now, at least n"""
    rng = np.random.default_rng(seed + 131 * n + n_max)
    orc = rng.uniform(-0.5, 0.3, (n, 128)).astype(F32)
    if n > 300:
        orc = (np.round(orc * 4096) / 4096).astype(F32)
    t_now = int(selection(orc, n_max, THR)[0].sum())
    return orc, n_max, THR, max(n, int(0.7 * t_now))
