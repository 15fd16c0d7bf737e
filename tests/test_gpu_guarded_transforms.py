"""The guarded two-precision selection (ADANERF_SAMPLING_GUARDED) under every sampler transform -- none (MSE), sigmoid
(BCEWithLogitsLoss), softmax (CrossEntropyLoss) -- against its guarantee: adanerf_compact_guarded(approx, exact) with |approx - exact| <= eps
on every raw value is the selection of `exact` bit for bit, re-evaluating only the rays the band cannot decide.  Inputs, classes and
checker: tests/selection_reference.py (guard section), themselves checked on the CPU by tests/test_guarded_transforms_cpu.py, which also
shows that the checker rejects a softmax band without max(p~), a sigmoid band of eps / 8, a raw band on transformed values, a pair bound
below 2 e under a transform, refined rays that keep approximate values, decided rays that carry exact ones and an off-by-one count.
Contexts are written from the synthetic_fixed8 scene with losses[0] replaced; the networks do not matter for the stage tests.

 a. soundness, no tolerance: counts, offsets, total and keys of G = compact_guarded(approx, exact) have the bits of CX = compact(exact) in the
    same context (pass 2 runs the code of adanerf_compact), for every (n_max in 1, 2, 4, 5, 8, 9, 16; eps in 0.01, 0.002; threshold)
    and every perturbation kind (rand, thr, cut; softmax also one).
 b. values, per ray: the kept values are CX's row or the row of CY = compact(approx), never a mixture; CX's on every ray of `must` (every
    row with a NaN or an infinity is one), CY's on every ray outside `may`.
 c. count: must.sum() <= refined <= may.sum(); without a transform refined == O.guard_undecided(approx).sum().
 d. monitor, in raw units under every transform: no violation, max_diff between the fp32 row maxima of |approx - exact| over must and over
    may, max_pair == 0 under a transform, nothing audited without an audit.
 e. audit under a transform (n_max 8, eps 0.002, period 16): errors beyond the band planted on rays that stay outside `may` are each
    counted in `violations` exactly once over the 16 phases, `audited` sums to a decided count between the two classes', the frame outputs
    are the same at every phase; planted selection-changing errors give exactly as many audit mismatches as planted rays whose CY row
    differs from CX's.
 f. position invariance: the case's rays permuted into 3 001 rays and its prefixes of 1, 31, 32, 33, 127, 128, 129 and 1 000 rays give every
    ray the bits of its base result (32-ray segments, 128-ray workgroups, the partial last mask word of refine_list_kernel).
 g. frames of the two transformed golden cases at 112 x 80, bf16: sampling="guarded" selects what sampling="split" selects, the monitor and
    the audit are silent, the kept values of the rays not refined are within the transformed band; again in batches of 1 000 rays; under the
    softmax guard_eps = 1 refines every ray and gives the split engine's frame byte for byte (no accepted band covers every sigmoid ray:
    the identical selection is all that is asked there).
The input conditions (<= 1 % borderline rays, >= 5 % outside may, >= 5 % inside must) are asserted again where the inputs are built.
Measured quantities: profiles/guarded_transforms_measured.log.

Kernels and the cases that reach them (every one under all three transforms):
  adanerf_compact_guarded
    select_rows_kernel, pass 1 (guard band: guard_band_of / guard_pair_of / pair_select's undecided; guard_mask, guard_probe)
      pair_select<4>                 test_guarded_stage[*-n] n = 1, 2, 4              test_guarded_position_invariance[*-4]
      pair_select<8>                 n = 5, 8      test_guarded_audit[*]              test_guarded_position_invariance[*-8]
      pair_select<16>                n = 9, 16                                        test_guarded_position_invariance[*-16]
    refine_list_kernel               every case; partial last word: every case (R is no multiple of 32) and the prefixes of f.;
                                     audit_bits: test_guarded_audit[*]
    select_rows_kernel, pass 2 (pair_epilogue<REFINE>: row_load / pair_monitor / guard_flush, the audit's compare-only pair_emit)
                                     every case; audit entries: test_guarded_audit[*]
    expand_kernel                    every case (seg_shift 5)
  the sampling kernels' fused pass 1 / pass 2 (pair_epilogue in the sampling kernels, poll_guard)
                                     test_guarded_frames[*] (pair_select<8>: the golden cases have N = 8)"""
import dataclasses

import numpy as np
import pytest

import adanerf_oracle as O
import selection_reference as SR
from conftest import TRANSFORM_CASES, case_weights, load_case, record
from stage_reference import permuted
from test_gpu_selection_transforms import run_compact
from test_gpu_stage_kernels import PAD, Guarded, same_bits

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 2024
SENTINEL32 = 0xA5A5A5A5
PREFIXES = [1, 31, 32, 33, 127, 128, 129, 1000]
LONG = 3001


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def ctxs(tmp_path_factory):
    """one context per transform: the pair selection (no wave_select), as the guarded form needs"""
    z, meta, sc = load_case("synthetic_fixed8")
    out = {}
    for losses0 in SR.LOSSES:
        d = str(tmp_path_factory.mktemp("guard_" + losses0))
        O.write_model_dir(d, dataclasses.replace(sc, losses0=losses0), O.synthetic_weights(1))
        out[losses0] = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 8, 8), precision="fp32")
        out[losses0].init()
    yield out
    for r in out.values():
        r.close()


def zeroed(r, nbytes):
    """a Guarded whose body starts as zeros (the monitor is added to)"""
    g = Guarded(r, nbytes)
    a = np.full(PAD + g.n + PAD, 0xA5, np.uint8)
    a[PAD:PAD + g.n] = 0
    g.buf.upload(a)
    return g


def run_guarded(r, d_approx, d_exact, n, n_max, thr, eps, what, period=0, phase=0):
    """adanerf_compact_guarded with a monitor into exact-size outputs between canaries -> the dict of run_compact + refined, mon"""
    off, cnt, tot, ref = Guarded(r, n * 4), Guarded(r, n * 4), Guarded(r, 4), Guarded(r, 4)
    key, w = Guarded(r, n * n_max * 4), Guarded(r, n * n_max * 4)
    mon = zeroed(r, 20)
    r.compact_guarded(d_approx, d_exact, n, n_max, thr, eps, off.ptr, cnt.ptr, key.ptr, w.ptr, tot.ptr, ref.ptr, audit_period=period,
                      audit_phase=phase, monitor=mon.ptr)
    r.sync()
    g = dict(off=off.body(what + " offsets", np.int32), cnt=cnt.body(what + " counts", np.int32), total=int(tot.body(what + " total", np.int32)[0]),
             key=key.body(what + " keys", np.uint32), w=w.body(what + " weights", np.uint32), refined=int(ref.body(what + " refined", np.int32)[0]))
    m = mon.body(what + " monitor", np.uint32)
    g["mon"] = dict(max_diff=float(m[:1].view(F32)[0]), violations=int(m[1]), max_pair=float(m[2:3].view(F32)[0]), audit_mismatch=int(m[3]), audited=int(m[4]))
    c = g["cnt"].astype(np.int64)
    assert (c >= 1).all() and (c <= n_max).all(), what + ": a count outside 1..n_max"
    t = g["total"]
    assert t == int(c.sum()) and np.array_equal(g["off"], np.cumsum(c) - c), what + ": total / offsets"
    assert (g["key"][t:] == SENTINEL32).all() and (g["w"][t:] == SENTINEL32).all(), what + ": the unused tail was written"
    g["w"] = g["w"].view(F32)
    g["bins"], g["vals"] = SR.rows_of(g["off"], g["cnt"], g["key"], g["w"], n_max)
    return g


def classes(a, losses0, n_max, thr, eps, what):
    must, may = SR.guard_classes(a, losses0, n_max, thr, eps)
    return (must, may) + SR.assert_guard_conditions(must, may, what)


@pytest.mark.parametrize("n_max", SR.GUARD_N)
@pytest.mark.parametrize("losses0", SR.LOSSES)
def test_guarded_stage(ctxs, losses0, n_max):
    r = ctxs[losses0]
    for eps in SR.GUARD_EPS:
        for thr in SR.guard_thresholds(losses0):
            c = SR.guard_inputs(SEED, losses0, n_max, thr, eps)
            exact = c["exact"]
            n = exact.shape[0]
            assert n % 32 != 0
            d_exact = r.to_device(exact)
            CX = run_compact(r, d_exact, n, n_max, thr, "exact")
            for kind, a in c["approx"]:
                what = "%s n_max %d eps %g thr %g %s" % (losses0, n_max, eps, thr, kind)
                fin = np.isfinite(exact)
                assert (np.abs(a[fin].astype(np.float64) - exact[fin].astype(np.float64)) <= float(F32(eps))).all() and SR.same_nonfinite(a, exact)
                must, may, border, outside, inside = classes(a, losses0, n_max, thr, eps, what)
                exact_refined = None
                if losses0 == "MSE":
                    with np.errstate(all="ignore"):
                        exact_refined = int(O.guard_undecided(a, n_max, thr, eps).sum())
                d_approx = r.to_device(a)
                CY = run_compact(r, d_approx, n, n_max, thr, what + " approx")
                G = run_guarded(r, d_approx, d_exact, n, n_max, thr, eps, what)
                d_approx.free()
                print(what, "refined", G["refined"], "must", inside, "may", inside + border, G["mon"])
                record("guarded_transform_stage", losses0=losses0, n_max=n_max, eps=eps, thr=thr, kind=kind, rays=n, refined=G["refined"],
                       must=inside, borderline=border, outside=outside, row_max_must=SR.row_max_diff(a, exact, must),
                       row_max_may=SR.row_max_diff(a, exact, may), transform_bound=SR.transform_bound(a, losses0), **G["mon"])
                out = SR.check_guarded(losses0, a, exact, must, may, G, CX, CY, exact_refined)
                assert out["carried_exact"] > 0
            d_exact.free()


def plant(a, rows, col, delta, losses0, n_max, thr, eps):
    """a + delta at (rows, col[rows]) on the rows that stay outside `may` with it -> the planted array, the rows that carry the plant"""
    b = a.copy()
    b[rows, col[rows]] += F32(delta)
    may = SR.guard_classes(b, losses0, n_max, thr, eps)[1]
    stay = rows[~may[rows]]
    b = a.copy()
    b[stay, col[stay]] += F32(delta)
    return b, stay


@pytest.mark.parametrize("losses0", SR.LOSSES)
def test_guarded_audit(ctxs, losses0):
    r = ctxs[losses0]
    n_max, eps, thr, period = 8, 0.002, SR.THRESHOLDS[losses0], 16
    c = SR.guard_inputs(SEED, losses0, n_max, thr, eps)
    exact, a = c["exact"], c["approx"][0][1]
    n = exact.shape[0]
    must0, may0 = SR.guard_classes(a, losses0, n_max, thr, eps)
    rows = np.flatnonzero(~may0)
    d_exact = r.to_device(exact)
    CX = run_compact(r, d_exact, n, n_max, thr, "exact")
    # 1: a violated bound that changes no selection -- the row's smallest value lowered by 0.05
    # 2: an error that changes selections -- the largest value the approximate selection leaves out raised by 0.05
    kept = SR.kept_mask(*O.select_adaptive(O.oracle_transform(np.where(np.isfinite(a), a, F32(0)), losses0), n_max, thr)[:2])
    cols = {"beyond the band": (np.argmin(np.where(np.isfinite(a), a, np.inf), axis=1), -0.05),
            "selection-changing": (np.argmax(np.where(kept | ~np.isfinite(a), -np.inf, a), axis=1), 0.05)}
    for name, (col, delta) in cols.items():
        b, planted = plant(a, rows, col, delta, losses0, n_max, thr, eps)
        must, may = SR.guard_classes(b, losses0, n_max, thr, eps)
        others = np.setdiff1d(np.arange(n), planted)
        assert planted.size >= 0.05 * n and not may[planted].any() and np.array_equal(must[others], must0[others]) and np.array_equal(may[others], may0[others])
        what = "%s audit, %s" % (losses0, name)
        d_b = r.to_device(b)
        CY = run_compact(r, d_b, n, n_max, thr, what + " approx")
        wrong = (CY["cnt"] != CX["cnt"]) | (CY["bins"] != CX["bins"]).any(1)
        assert not (wrong & ~may)[others].any()      # soundness on everything that carries no plant
        base = run_guarded(r, d_b, d_exact, n, n_max, thr, eps, what + " no audit")
        assert base["mon"]["violations"] == 0 and base["mon"]["audited"] == 0 and base["mon"]["audit_mismatch"] == 0      # audit off: blind
        tot = dict(violations=0, audited=0, audit_mismatch=0)
        for phase in range(period):
            g = run_guarded(r, d_b, d_exact, n, n_max, thr, eps, what + " phase %d" % phase, period=period, phase=phase)
            for k in ("off", "cnt", "total", "key", "w"):      # compare-only: nothing the frame is made of moves
                assert same_bits(np.asarray(g[k]), np.asarray(base[k])), "%s: %s moves with the audit phase %d" % (what, k, phase)
            aud = ((np.arange(n) % 32 - phase - np.arange(n) // 32) & (period - 1)) == 0
            assert int((must | aud).sum()) <= g["refined"] <= int((may | aud).sum())
            for k in tot:
                tot[k] += g["mon"][k]
        d_b.free()
        print(what, "planted", planted.size, "wrong among them", int(wrong[planted].sum()), tot)
        record("guarded_transform_audit", losses0=losses0, plant=name, rays=n, planted=int(planted.size), wrong=int(wrong[planted].sum()), **tot)
        assert tot["violations"] == planted.size, "%s: %d violations over the rotation, %d planted rays" % (what, tot["violations"], planted.size)
        assert int((~may).sum()) <= tot["audited"] <= int((~must).sum())
        assert tot["audit_mismatch"] == int(wrong[planted].sum()), "%s: %d mismatches, %d planted rays select wrongly" % (what, tot["audit_mismatch"], int(wrong[planted].sum()))
        assert name == "beyond the band" or wrong[planted].sum() >= 20
    d_exact.free()


@pytest.mark.parametrize("n_max", [4, 8, 16])
@pytest.mark.parametrize("losses0", SR.LOSSES)
def test_guarded_position_invariance(ctxs, losses0, n_max):
    r = ctxs[losses0]
    eps, thr = 0.01, SR.THRESHOLDS[losses0]
    c = SR.guard_inputs(SEED, losses0, n_max, thr, eps)
    kind, a = c["approx"][-1]      # cut / one: the band rows of both types sit on their placements
    exact = c["exact"]
    B = exact.shape[0]
    must, may = SR.guard_classes(a, losses0, n_max, thr, eps)
    tag = "%s n_max %d %s" % (losses0, n_max, kind)
    d_a, d_x = r.to_device(a), r.to_device(exact)
    base = run_guarded(r, d_a, d_x, B, n_max, thr, eps, tag + " base")
    d_a.free()
    d_x.free()
    ids = permuted(LONG, B)
    assert np.unique(ids).size == B
    d_a, d_x = r.to_device(np.ascontiguousarray(a[ids])), r.to_device(np.ascontiguousarray(exact[ids]))
    for n in [LONG] + PREFIXES:
        g = run_guarded(r, d_a, d_x, n, n_max, thr, eps, tag + " %d rays" % n)
        what = tag + " %d rays" % n
        assert np.array_equal(g["cnt"], base["cnt"][ids[:n]]), what + ": counts"
        assert np.array_equal(g["bins"], base["bins"][ids[:n]]), what + ": bins"
        assert same_bits(g["vals"], base["vals"][ids[:n]]), what + ": kept values"
        assert np.array_equal(g["key"][:g["total"]] >> 7, np.repeat(np.arange(n, dtype=np.uint32), g["cnt"])), what + ": ray ids of the keys"
        assert int(must[ids[:n]].sum()) <= g["refined"] <= int(may[ids[:n]].sum()), what + ": refined"
        assert g["mon"]["violations"] == 0 and g["mon"]["audited"] == 0
    d_a.free()
    d_x.free()


# ---- whole frames -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", TRANSFORM_CASES)
def test_guarded_frames(name, tmp_path):
    z, meta, sc = load_case(name)
    d = str(tmp_path / "m")
    O.write_model_dir(d, sc, case_weights(meta))
    w, h = 112, 80
    n_max = sc.num_samples
    soft = sc.losses0 in SR.SOFTMAX
    # what a correct fp32 transform may differ by between the two engines' kept values, beside the band: the reference's own bound on the
    # stage inputs (selection_reference.transform_bound), on either value
    bound = SR.transform_bound(SR.selection_inputs(SEED, sc.losses0)["raw"], sc.losses0)

    def run(bs=-1, **kw):
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h, batch_size=bs), precision="bf16", **kw) as r:
            r.set_camera(z["pose"], z["rot"])
            rgb, rgba, st = r.render_numpy()
            nb = r.info.batch_rays
            last = (w * h) - ((w * h - 1) // nb) * nb
            g = dict(cnt=r.buffer(R.BUF_RAY_COUNTS, np.int32, (last,)), off=r.buffer(R.BUF_RAY_OFFSETS, np.int32, (last,)),
                     total=int(r.buffer(R.BUF_TOTAL, np.int32, (1,))[0]), rgb=rgb, rgba=rgba, samples=int(st.total_samples))
            g["key"], g["w"] = r.buffer(R.BUF_SAMPLE_KEY, np.uint32, (g["total"],)), r.buffer(R.BUF_SAMPLE_W, F32, (g["total"],))
            assert st.sampling_overflow == 0
            r.refresh_info()
            g["st"] = dict(refined=int(st.rays_refined), seen=float(st.guard_max_seen), violations=int(st.guard_violations), audited=int(st.guard_audited),
                           mismatch=int(st.guard_audit_mismatch), eps=float(r.info.guard_eps), eps_pair=float(r.info.guard_eps_pair))
            return g

    def same_selection(a, b, what):
        for k in ("samples", "cnt", "off", "total", "key"):
            assert same_bits(np.asarray(a[k]), np.asarray(b[k])), "%s %s: %s of the guarded and the split frame differ" % (name, what, k)

    for bs in (-1, 1000):
        what = "whole frame" if bs < 0 else "batches of %d" % bs
        split, guard = run(bs, sampling="split"), run(bs, sampling="guarded")
        same_selection(guard, split, what)
        s = guard["st"]
        print(name, what, s)
        assert split["st"]["refined"] == 0
        assert s["violations"] == 0 and s["seen"] <= s["eps"] and s["mismatch"] == 0 and s["audited"] > 0, (what, s)
        assert 0 < s["refined"] < w * h, (what, s)
        assert s["eps_pair"] == float(F32(2) * F32(s["eps"])), (what, s)
        # the kept values: the split engine's on the refined rays, inside the transformed band on the others
        bins, vg = SR.rows_of(guard["off"], guard["cnt"], guard["key"], guard["w"], n_max)
        _, vs = SR.rows_of(split["off"], split["cnt"], split["key"], split["w"], n_max)
        f = SR.guard_factor(sc.losses0, s["eps"])
        band = f * np.abs(vg).max(1, keepdims=True).astype(np.float64) if soft else f      # the row maximum is always kept
        diff = np.abs(vg.astype(np.float64) - vs.astype(np.float64))
        tol = band + 2.0 * (bound * np.maximum(np.abs(vg), np.abs(vs)) + SR.FLOOR)
        assert (diff <= tol).all(), "%s %s: a kept value differs from the split engine's by %g of the band" % (name, what, float((diff / tol).max()))
        record("guarded_transform_frame", case=name, batch=bs, rays=w * h, refined_frac=s["refined"] / (w * h), max_value_diff_over_band=float((diff / tol).max()),
               frame_identical=bool(same_bits(guard["rgba"], split["rgba"])), **s)
        if bs < 0:
            whole = split
    wide = run(sampling="guarded", guard_eps=1.0)
    same_selection(wide, whole, "guard_eps 1")
    assert wide["st"]["eps"] == 1.0 and wide["st"]["violations"] == 0 and wide["st"]["mismatch"] == 0
    record("guarded_transform_frame_wide", case=name, rays=w * h, **wide["st"])
    if soft:      # exp(2) - 1 > 1: the band covers every probability; the whole frame is the split engine's
        assert wide["st"]["refined"] == w * h
        for k in ("w", "rgb", "rgba"):
            assert same_bits(np.asarray(wide[k]), np.asarray(whole[k])), "%s guard_eps 1: %s is not the split engine's" % (name, k)
