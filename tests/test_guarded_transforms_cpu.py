"""The guarded two-precision selection under every sampler transform, on the CPU: the inputs, the classes and the checker that
tests/test_gpu_guarded_transforms.py holds the device to (selection_reference.py, guard section), checked against the oracle's fp32
restatement of the rule before any kernel runs.

 soundness   on every (transform, n_max, eps, thr) case and perturbation kind the fp32 numpy rule (O.guard_undecided on
             O.oracle_transform(approx)) leaves no decided ray whose selection differs between approx and exact
 teeth       the same inputs convict a band that is too narrow: with the rule at 0.5 eps and at 0.8 eps (perturbation still eps) at least
             8 rays of every case are decided and wrong.  A condition on the inputs.  Under the softmax with n_max = 1 no input can have
             teeth (selection_reference: a threshold row keeps the arg-max either way; the ratio of two probabilities moves by exp(2 eps)
             while the pair bound allows exp(4 eps)): there the test asserts that nothing is unsound at either scale, which is what the
             argument predicts, and the case stays in the GPU file for its must / may classes.
 conditions  per (case, kind): <= 1 % borderline rays, >= 5 % outside may, >= 5 % inside must; must <= the fp32 rule <= may; the band rows
             have the class they were built for under their own kind; without a transform must == may == O.guard_undecided
 rejection   check_guarded accepts the emulated correct result of every kind and rejects each emulated faulty device"""
import numpy as np
import pytest

import adanerf_oracle as O
import selection_reference as SR

F32 = np.float32
SEED = 2024
CASES = [(l, n, eps, thr) for l in SR.LOSSES for n in SR.GUARD_N for eps in SR.GUARD_EPS for thr in SR.guard_thresholds(l)]


_INPUTS = {}


def _inputs(losses0, n_max, eps, thr):
    """built once per case and shared; nothing writes to them"""
    key = (losses0, n_max, eps, thr)
    if key not in _INPUTS:
        _INPUTS[key] = SR.guard_inputs(SEED, losses0, n_max, thr, eps)
    return _INPUTS[key]


def _rule(a, losses0, n_max, thr, eps):
    with np.errstate(all="ignore"):
        ya = O.oracle_transform(a, losses0)
        return ya, O.guard_undecided(ya, n_max, thr, eps, SR.TRANSFORM_NAME[losses0]) | ~np.isfinite(a).all(1)


def _select(y, n_max, thr):
    with np.errstate(all="ignore"):
        c, b, _ = O.select_adaptive(y, n_max, thr)
    return c, b


@pytest.mark.parametrize("losses0,n_max,eps,thr", CASES)
def test_inputs_are_sound_have_teeth_and_meet_their_conditions(losses0, n_max, eps, thr):
    c = _inputs(losses0, n_max, eps, thr)
    exact = c["exact"]
    R = exact.shape[0]
    assert 1000 <= R <= 1150
    with np.errstate(all="ignore"):
        cx, bx = _select(O.oracle_transform(exact, losses0), n_max, thr)
    kinds = [k for k, _ in c["approx"]]
    assert kinds == ["rand", "thr", "cut"] + (["one"] if losses0 in SR.SOFTMAX else [])
    teeth = {0.5: np.zeros(R, bool), 0.8: np.zeros(R, bool)}
    for kind, a in c["approx"]:
        what = "%s n_max %d eps %g thr %g %s" % (losses0, n_max, eps, thr, kind)
        fin = np.isfinite(exact)
        assert (np.abs(a[fin].astype(np.float64) - exact[fin].astype(np.float64)) <= float(F32(eps))).all() and SR.same_nonfinite(a, exact)
        ya, und = _rule(a, losses0, n_max, thr, eps)
        ca, ba = _select(ya, n_max, thr)
        differs = (ca != cx) | (ba != bx).any(1)
        assert not (differs & ~und).any(), "%s: decided rays %s select differently from exact" % (what, np.flatnonzero(differs & ~und)[:8].tolist())
        must, may = SR.guard_classes(a, losses0, n_max, thr, eps)
        SR.assert_guard_conditions(must, may, what)
        assert (must <= und).all() and (und <= may).all(), what + ": the fp32 rule is not between must and may"
        if losses0 == "MSE":
            with np.errstate(all="ignore"):
                assert np.array_equal(must, may) and np.array_equal(must, O.guard_undecided(a, n_max, thr, eps))
        for k2, rows, cls in c["expect"]:
            if k2 == kind:
                assert rows.size and (must[rows].all() if cls == "must" else not may[rows].any()), "%s: band rows built to be %s are not" % (what, cls)
        for scale in teeth:
            teeth[scale] |= differs & ~_rule(a, losses0, n_max, thr, scale * eps)[1]
    counts = {s: int(t.sum()) for s, t in teeth.items()}
    if losses0 in SR.SOFTMAX and n_max == 1:
        assert counts == {0.5: 0, 0.8: 0}, "softmax, n_max 1: unsound rays %r where the argument says there can be none" % counts
    else:
        assert min(counts.values()) >= 8, "%s n_max %d eps %g thr %g: unsound rays at (0.5 eps, 0.8 eps): %r, need 8" % (losses0, n_max, eps, thr, counts)


def _faulty_bands(losses0, ya, n_max, thr, eps):
    """{fault: undecided [R]} of kernels that carry the raw band through the transform wrongly"""
    R = ya.shape[0]
    full = lambda v: np.full(R, F32(v), F32)
    out = {}
    with np.errstate(all="ignore"):
        c0 = ya.max(1)
    f = F32(SR.guard_factor(losses0, eps))
    if losses0 in SR.SOFTMAX:
        out["softmax band without max(p~)"] = SR.rule32(ya, n_max, thr, full(f))
        e = (f * c0).astype(F32)
    else:
        e = full(f)
    if losses0 == "BCEWithLogitsLoss":
        out["sigmoid band eps / 8"] = SR.rule32(ya, n_max, thr, full(0.125 * eps))
    if losses0 != "MSE":
        out["raw band on transformed values"] = SR.rule32(ya, n_max, thr, full(eps))
        out["pair bound below 2 e under a transform"] = SR.rule32(ya, n_max, thr, e, (F32(1.2) * e).astype(F32))
    return out


@pytest.mark.parametrize("losses0,n_max,eps,thr", [c for c in CASES if c[1] in (2, 8, 16)])
def test_checker_accepts_the_rule_and_rejects_faulty_devices(losses0, n_max, eps, thr):
    c = _inputs(losses0, n_max, eps, thr)
    exact = c["exact"]
    rejected = {}
    for kind, a in c["approx"]:
        must, may = SR.guard_classes(a, losses0, n_max, thr, eps)
        ya, und = _rule(a, losses0, n_max, thr, eps)
        exact_refined = int(und.sum()) if losses0 == "MSE" else None
        G, CX, CY = SR.emulate_guarded(losses0, a, exact, n_max, thr, eps)
        out = SR.check_guarded(losses0, a, exact, must, may, G, CX, CY, exact_refined)
        assert out["refined"] == int(und.sum()) and out["carried_exact"] > 0
        faulty = [(name, dict(undecided=u)) for name, u in _faulty_bands(losses0, ya, n_max, thr, eps).items()]
        faulty += [(name, dict(fault=name)) for name in ("refined keeps approx", "decided carries exact")]
        for name, kw in faulty:
            G, CX, CY = SR.emulate_guarded(losses0, a, exact, n_max, thr, eps, **kw)
            try:
                SR.check_guarded(losses0, a, exact, must, may, G, CX, CY, exact_refined)
            except AssertionError:
                rejected.setdefault(name, []).append(kind)
            else:
                rejected.setdefault(name, [])
        # an off-by-one count: pinned exactly without a transform, to the class counts otherwise
        for refined in ([int(und.sum()) + 1, int(und.sum()) - 1] if losses0 == "MSE" else [int(may.sum()) + 1, int(must.sum()) - 1]):
            G, CX, CY = SR.emulate_guarded(losses0, a, exact, n_max, thr, eps)
            G["refined"] = refined
            with pytest.raises(AssertionError, match="refined"):
                SR.check_guarded(losses0, a, exact, must, may, G, CX, CY, exact_refined)
        G, CX, CY = SR.emulate_guarded(losses0, a, exact, n_max, thr, eps)
        G["mon"]["max_pair"] = 0.004      # a pair statistic where no pair bound is in use
        if losses0 != "MSE":
            with pytest.raises(AssertionError, match="pair statistic"):
                SR.check_guarded(losses0, a, exact, must, may, G, CX, CY, exact_refined)
    # the GPU test runs every kind of a case: a faulty device fails the case when one kind convicts it; the value faults show in every kind
    assert all(rejected.values()), "not rejected under any kind: %s" % [k for k, v in rejected.items() if not v]
    for name in ("refined keeps approx", "decided carries exact"):
        assert len(rejected[name]) == len(c["approx"]), "%s passed under a kind: only %s reject it" % (name, rejected[name])
