"""tests/selection_reference.py on the CPU: the fp32 numpy restatement of the transformed selection, in both summation orders the
device uses for the softmax, passes the checker on every input and at every threshold the GPU tests run (test_gpu_selection_transforms.py);
the reference's own selections pass; the checker rejects every corruption it is there to find; the inputs meet the conditions the
GPU tests rely on (every count occurs, the fallback occurs, almost every ray is decided with margin)."""
import numpy as np
import pytest

import adanerf_oracle as O
import selection_reference as SR
from conftest import TRANSFORM_CASES, load_case

F32 = np.float32
N_MAX = [1, 3, 8, 16, 33, 128]
_CACHE = {}


def inputs(losses0):
    if losses0 not in _CACHE:
        c = SR.selection_inputs(2024, losses0)
        c["bound"] = SR.transform_bound(c["raw"], losses0)
        with np.errstate(all="ignore"):
            c["v32"] = {"wave": O.oracle_transform(c["raw"], losses0), "pair": SR.transform32_pair(c["raw"], losses0)}
        _CACHE[losses0] = c
    return _CACHE[losses0]


def select32(v32, n_max, thr):
    with np.errstate(all="ignore"):
        return O.select_adaptive(v32, n_max, thr)


@pytest.mark.parametrize("losses0", SR.LOSSES)
def test_bounds_come_from_the_reference(losses0):
    c = inputs(losses0)
    if losses0 == "MSE":
        assert c["bound"] == 0.0
    else:      # a handful of fp32 ulps: expf, one division, and for the softmax a sum of 128 terms
        assert 2.0 ** -25 < c["bound"] < 64 * 2.0 ** -24, c["bound"]
    assert 950 <= c["raw"].shape[0] <= 1050


@pytest.mark.parametrize("order", ["wave", "pair"])
@pytest.mark.parametrize("n_max", N_MAX)
@pytest.mark.parametrize("losses0", SR.LOSSES)
def test_fp32_restatement_passes(losses0, n_max, order):
    """numpy's pairwise sum stands for oracle_transform_wave's wave reduction, transform32_pair is pair_epilogue's order"""
    c = inputs(losses0)
    for thr in SR.thresholds(losses0):
        cnt, bins, w = select32(c["v32"][order], n_max, thr)
        out = SR.check_selection(c["raw"], losses0, n_max, thr, cnt, bins, w, c["bound"])
        assert out["worst_residual"] <= c["bound"]
        SR.assert_edges(c, n_max, thr, cnt, bins, "%s %s" % (losses0, order))


def test_the_two_softmax_orders_differ():
    """or the pair-against-wave rule of the GPU tests would be a bit-for-bit rule in disguise"""
    c = inputs("CrossEntropyLoss")
    a, b = c["v32"]["wave"], c["v32"]["pair"]
    ok = np.isfinite(a) & np.isfinite(b)
    assert 0.2 < (a[ok] != b[ok]).mean() < 0.9
    with np.errstate(all="ignore"):
        assert np.nanmax(np.abs(a[ok].astype(np.float64) - b[ok]) / np.maximum(np.abs(a[ok]), SR.FLOOR)) <= c["bound"]


@pytest.mark.parametrize("name", TRANSFORM_CASES)
def test_the_references_own_selections_pass(name):
    z, meta, sc = load_case(name)
    raw = z["oracle_out"]
    bound = SR.transform_bound(raw, sc.losses0)
    out = SR.check_selection(raw, sc.losses0, sc.num_samples, sc.threshold, z["sel_count"], z["sel_bins"], z["sel_weight"], bound)
    assert out["undecided"] <= 0.01 * out["rays"]


@pytest.mark.parametrize("losses0", SR.LOSSES)
def test_input_conditions(losses0):
    c = inputs(losses0)
    raw, kind = c["raw"], c["kind"]
    rnd, qnt = kind == "random", kind == "quantised"
    v = SR.transform64(raw, losses0)
    on_half = (SR.tie_keys(raw, losses0) == SR.tie_keys(np.full((1, 1), 0.5 if losses0 == "MSE" else 0.0, F32), losses0)).any(1)
    assert (qnt & on_half).sum() > 100 and (qnt & ~on_half).sum() > 20
    for thr in SR.thresholds(losses0):
        t = float(F32(thr))
        reach = (v >= t).sum(1)
        main = thr == SR.THRESHOLDS[losses0]
        if main and losses0 != "CrossEntropyLoss":
            for n_max in range(1, 17):
                got = set(np.minimum(np.maximum(reach[rnd | qnt], 1), n_max).tolist())
                assert got == set(range(1, n_max + 1)), (losses0, n_max, sorted(got))
        # the fallback: no softmax of 128 values at these scales stays below 0.012 everywhere, so the softmax rows meet it at 0.5
        if main if losses0 != "CrossEntropyLoss" else thr == 0.5:
            assert 0.02 <= (reach[rnd] == 0).mean() <= 0.98, (losses0, (reach[rnd] == 0).mean())
        for n_max in N_MAX + [2, 4, 5, 9, 17, 32, 64, 127]:
            cnt, bins, w = select32(c["v32"]["wave"], n_max, thr)
            dec = SR.verdict(raw, losses0, n_max, thr, cnt, bins, w, c["bound"])["decided"]
            assert (~dec[rnd]).mean() <= 0.01, (losses0, thr, n_max, (~dec[rnd]).mean())
            placed = on_half if (thr == 0.5 and losses0 != "CrossEntropyLoss") else np.zeros_like(on_half)
            assert dec[qnt & ~placed].all(), (losses0, thr, n_max, np.flatnonzero(qnt & ~placed & ~dec)[:8])
            if thr == 0.5 and losses0 != "CrossEntropyLoss":
                assert not dec[qnt & placed].any()


# ---- the checker finds what it is there to find --------------------------------------------------------------------------------------

def mutate(c, losses0, n_max, thr, change, rows):
    """applies change(K row, ray) -> new kept set (or None) to the fp32 restatement's selection on `rows`; -> the rays the checker calls bad"""
    v32 = c["v32"]["wave"]
    cnt, bins, w = select32(v32, n_max, thr)
    K = SR.kept_mask(cnt, bins)
    done = []
    for r in rows:
        k = change(K[r].copy(), r)
        if k is not None:
            K[r] = k
            done.append(r)
    cnt, bins, w = SR.pack(K, v32, n_max)
    return np.array(done, np.int64), SR.verdict(c["raw"], losses0, n_max, thr, cnt, bins, w, c["bound"])


@pytest.mark.parametrize("losses0", SR.LOSSES)
def test_checker_rejects_corrupted_selections(losses0):
    c = inputs(losses0)
    raw, kind = c["raw"], c["kind"]
    n_max, thr = 8, SR.THRESHOLDS[losses0]
    v = SR.transform64(raw, losses0)
    vn = np.where(np.isnan(v), -np.inf, v)
    v32 = c["v32"]["wave"]
    cnt0, bins0, w0 = select32(v32, n_max, thr)
    base = SR.verdict(raw, losses0, n_max, thr, cnt0, bins0, w0, c["bound"])
    assert not base["bad"].any()
    dec = base["decided"] & ~np.isnan(v).all(1)
    rows = np.flatnonzero(dec)
    key = SR.tie_keys(raw, losses0)

    def every_kind(done, min_kinds=("random", "quantised", "edge")):
        assert set(min_kinds) <= set(kind[done].tolist()), (set(kind[done].tolist()), min_kinds)

    def all_bad(done, res, reason=None):
        assert done.size and res["bad"][done].all(), np.flatnonzero(~res["bad"][done])[:8]
        assert not np.delete(res["bad"], done).any()      # and nobody else
        if reason:
            assert res["reasons"][reason][done].all(), reason

    # 1. the best kept bin swapped for the best left-out one
    def swap_best(K, r):
        out_ = np.flatnonzero(~K & ~np.isnan(v[r]))
        if out_.size == 0:
            return None
        K[np.flatnonzero(K)[np.argmax(vn[r][K])]] = False
        K[out_[np.argmax(vn[r][out_])]] = True
        return K
    done, res = mutate(c, losses0, n_max, thr, swap_best, rows)
    all_bad(done, res)
    every_kind(done)

    # 2. a tie resolved to the higher bin: a kept bin gives way to a left-out bin of equal input above it
    def tie_up(K, r):
        for k in np.flatnonzero(K):
            j = np.flatnonzero(~K & (key[r] == key[r, k]) & (np.arange(128) > k))
            if j.size:
                K[k], K[j[0]] = False, True
                return K
        return None
    done, res = mutate(c, losses0, n_max, thr, tie_up, np.flatnonzero(~np.isnan(v).all(1)))      # an all-NaN row has its own rule (5.)
    all_bad(done, res, "tie resolved to the higher bin")
    every_kind(done, ("quantised", "edge"))

    # 3. a stale value: the raw output (without a transform: the neighbouring bin's) where the ranked value belongs
    w = w0.copy()
    other = raw[np.arange(raw.shape[0]), bins0[:, 0]] if losses0 != "MSE" else raw[np.arange(raw.shape[0]), (bins0[:, 0] + 1) % 128]
    with np.errstate(all="ignore"):
        differs = np.isfinite(other) & np.isfinite(w[:, 0]) & ~(np.abs(other.astype(np.float64) - v[np.arange(raw.shape[0]), bins0[:, 0]]) <= 1e-3)
    w[differs, 0] = other[differs]
    res = SR.verdict(raw, losses0, n_max, thr, cnt0, bins0, w, c["bound"])
    done = np.flatnonzero(differs)
    all_bad(done, res, "kept value outside the bound")
    every_kind(done)

    # 4. a count off by one: the worst kept bin dropped / the best left-out bin added
    def drop_worst(K, r):
        if K.sum() < 2:
            return None
        K[np.flatnonzero(K)[np.argmin(vn[r][K])]] = False
        return K
    done, res = mutate(c, losses0, n_max, thr, drop_worst, rows)
    all_bad(done, res)
    every_kind(done)

    def add_best(K, r):
        out_ = np.flatnonzero(~K & ~np.isnan(v[r]))
        if K.sum() >= n_max or out_.size == 0:
            return None
        K[out_[np.argmax(vn[r][out_])]] = True
        return K
    done, res = mutate(c, losses0, n_max, thr, add_best, rows)
    all_bad(done, res)
    every_kind(done)
    bad_cnt = cnt0.copy()
    bad_cnt[cnt0 == n_max] += 1      # and a count beyond n_max as such
    res = SR.verdict(raw, losses0, n_max, thr, bad_cnt, bins0, w0, c["bound"])
    all_bad(np.flatnonzero(cnt0 == n_max), res, "count outside 1..n_max")
    res = SR.verdict(raw, losses0, n_max, thr, np.zeros_like(cnt0), bins0, w0, c["bound"])
    assert res["bad"].all()

    # 5. a kept NaN
    def keep_nan(K, r):
        nn = np.flatnonzero(np.isnan(v[r]) & ~K)
        if nn.size == 0 or np.isnan(v[r]).all():
            return None
        K[np.flatnonzero(K)[0]] = False
        K[nn[0]] = True
        return K
    if losses0 not in SR.SOFTMAX:      # a NaN makes a whole softmax row NaN
        done, res = mutate(c, losses0, n_max, thr, keep_nan, np.arange(raw.shape[0]))
        all_bad(done, res, "kept bin with a NaN value")
    allnan = np.flatnonzero(np.isnan(v).all(1))
    b = bins0.copy()
    b[allnan, 0] = 5      # an all-NaN row that keeps another bin than 0
    res = SR.verdict(raw, losses0, n_max, thr, cnt0, b, w0, c["bound"])
    all_bad(allnan, res, "all-NaN row does not keep bin 0 alone")

    # 6. two bins out of order
    two = np.flatnonzero(cnt0 >= 2)
    b, w = bins0.copy(), w0.copy()
    b[two, 0], b[two, 1] = bins0[two, 1], bins0[two, 0]
    w[two, 0], w[two, 1] = w0[two, 1], w0[two, 0]
    res = SR.verdict(raw, losses0, n_max, thr, cnt0, b, w, c["bound"])
    all_bad(two, res, "bins do not ascend")
    every_kind(two)

    # 7. the fallback taken although values clear the threshold
    def only_argmax(K, r):
        if K.sum() < 2:
            return None
        K[:] = False
        K[np.argmax(vn[r])] = True
        return K
    done, res = mutate(c, losses0, n_max, thr, only_argmax, rows)
    all_bad(done, res)
    every_kind(done)

    # 8. the saturated sigmoid answered with the largest logits
    if losses0 == "BCEWithLogitsLoss":
        sat = [row for row, name, _ in c["edges"] if name == "saturated"][0]
        for n in (1, 8, 16):
            def largest(K, r):
                K[:] = False
                K[30 - n:30] = True
                return K
            done, res = mutate(c, losses0, n, thr, largest, [sat])
            all_bad(done, res, "tie resolved to the higher bin")
