"""The adaptive selection (stage A4) under the sampler's transform -- sigmoid (losses[0] = BCEWithLogitsLoss), softmax
(CrossEntropyLoss), none (MSE) -- against the fp64 restatement of tests/selection_reference.py, through adanerf_compact /
adanerf_compact_budget and through whole frames.  Models are written from the synthetic_fixed8 scene; the networks do not matter here.

 a. accuracy: selection_reference.check_selection on the base set (about 1 000 rows: random, quantised with many equal logits, logits
    near 1e4, and the determinate edge rows -- saturated sigmoids, exact 0.5 and 1/128, one-hot and -inf softmax rows, NaN, +-inf),
    no ray excused, at the transform's threshold (0.2 / 0.6 / 0.012) and at the exact-boundary thresholds 0.5, 1/128 and
    nextafter(1/128, 1); the edge rows' kept bins asserted exactly.  Bound: selection_reference.transform_bound -- twice the fp32 numpy
    oracle's relative residual against fp64 on the same rows; the device's residuals are recorded beside it
    (profiles/selection_transforms_measured.log).
 b. layout: counts, offsets, total and the keys' ray ids exact, the unused tail of key and weight untouched, every output between two
    4 KiB canary regions.
 c. position invariance, no tolerance: every occurrence of a base ray in a permuted list of 3 001 rays and in every prefix of it of
    1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257 and 1 000 rays has the bits of its base-set result (16-ray waves and
    64-ray workgroups of select_kernel, 32-ray segments and 128-ray workgroups of select_rows_kernel, 256-ray workgroups of
    expand_kernel); zero rays write nothing.
 d. pair against wave, n_max <= 16: without a transform and under the sigmoid everything is bit-identical (one expression, built with
    -ffp-contract=off).  Under the softmax the two kernels sum the 128 exponentials in different orders (a wave reduction / two serial
    sums of 64), so they owe each other: each passes the checker, counts and bins are equal on every ray the checker reports as decided
    with margin, and the kept values of a bin both keep differ by at most the bound.
 e. fused against separate launches: whole frames of the two transformed golden cases; the fused epilogue and the pair launch
    (keep_oracle) are bit-identical, the wave launch is held to d.
 f. the per-ray budget trim under a transform: ray r of adanerf_compact_budget has the bits of ray r of adanerf_compact(n_r, thr_r) in
    the same context.
 g. dense mode (threshold 0) with a transformed model returns the raw outputs.

Kernels and the cases that reach them (every one under all three transforms):
  launch_compact, n_max <= 16 and no ADANERF_FLAG_WAVE_SELECT
    select_rows_kernel / pair_epilogue
      pair_select<4>                 test_selection_accuracy[pair-n-*] n = 1, 2, 4        test_position_invariance[pair-4-*]
      pair_select<8>                 n = 5, 8                                             test_position_invariance[pair-8-*]
      pair_select<16>                n = 9, 16                                            test_position_invariance[pair-16-*]
  launch_compact, ADANERF_FLAG_WAVE_SELECT (or n_max > 16)
    select_kernel / oracle_transform_wave / select_ray
                                     test_selection_accuracy[wave-n-*] n = 1, 4, 8, 16, 17, 32, 33, 64, 127, 128
                                     test_position_invariance[wave-n-*] n = 8, 33, 128
  expand_kernel                      every case above (seg_shift 5 behind the pair kernel, 6 behind select_kernel)
  fused epilogue (pair_epilogue in the sampling kernel)
                                     test_fused_pair_and_wave_frames[*] (pair_select<8>: the golden cases have N = 8)
  launch_trim
    trim_rows_kernel                 test_budget_trim_under_a_transform[pair-8-*], [wave-8-*]
    trim_rows_wave_kernel            test_budget_trim_under_a_transform[wave-32-*]
  dense_expand_kernel                test_dense_mode_returns_the_raw_outputs"""
import dataclasses

import numpy as np
import pytest

import adanerf_oracle as O
import selection_reference as SR
from conftest import TRANSFORM_CASES, case_weights, load_case, record
from stage_reference import permuted
from test_gpu_stage_kernels import Guarded, same_bits

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

F32 = np.float32
PAIR_N = [1, 2, 4, 5, 8, 9, 16]                        # both sides of the pair_select<4 | 8 | 16> edges
WAVE_N = [1, 4, 8, 16, 17, 32, 33, 64, 127, 128]
KERNEL_N = [("pair", n) for n in PAIR_N] + [("wave", n) for n in WAVE_N]
POSITION_N = [("pair", 4), ("pair", 8), ("pair", 16), ("wave", 8), ("wave", 33), ("wave", 128)]
PREFIXES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
LONG = 3001
SENTINEL32 = 0xA5A5A5A5
_INPUTS = {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


def inputs(losses0):
    if losses0 not in _INPUTS:
        c = SR.selection_inputs(2024, losses0)
        c["bound"] = SR.transform_bound(c["raw"], losses0)
        _INPUTS[losses0] = c
    return _INPUTS[losses0]


@pytest.fixture(scope="module")
def ctxs(tmp_path_factory):
    """one context per (transform, selection kernel)"""
    z, meta, sc = load_case("synthetic_fixed8")
    out = {}
    for losses0 in SR.LOSSES:
        d = str(tmp_path_factory.mktemp("sel_" + losses0))
        O.write_model_dir(d, dataclasses.replace(sc, losses0=losses0), O.synthetic_weights(1))
        for kernel in ("pair", "wave"):
            out[losses0, kernel] = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 8, 8), precision="fp32", wave_select=kernel == "wave")
            out[losses0, kernel].init()
    yield out
    for r in out.values():
        r.close()


def run_compact(r, d_orc, n, n_max, thr, what, maps=None):
    """adanerf_compact (maps: (d_n_map, d_thr_map) -> adanerf_compact_budget) into exact-size guarded outputs; layout b. asserted
    -> dict(cnt, off, total, key, w, bins [n, n_max], vals [n, n_max])"""
    off, cnt, tot = Guarded(r, n * 4), Guarded(r, n * 4), Guarded(r, 4)
    key, w = Guarded(r, n * n_max * 4), Guarded(r, n * n_max * 4)
    if maps is None:
        r.compact(d_orc, n, n_max, thr, off.ptr, cnt.ptr, key.ptr, w.ptr, tot.ptr)
    else:
        r.compact_budget(d_orc, n, n_max, thr, maps[0], maps[1], off.ptr, cnt.ptr, key.ptr, w.ptr, tot.ptr)
    r.sync()
    g = dict(off=off.body(what + " offsets", np.int32), cnt=cnt.body(what + " counts", np.int32), total=int(tot.body(what + " total", np.int32)[0]),
             key=key.body(what + " keys", np.uint32), w=w.body(what + " weights", np.uint32))
    c = g["cnt"].astype(np.int64)
    assert (c >= 1).all() and (c <= n_max).all(), what + ": a count outside 1..n_max"
    assert g["total"] == int(c.sum()), what + ": total"
    assert np.array_equal(g["off"], np.cumsum(c) - c), what + ": offsets"
    t = g["total"]
    assert np.array_equal(g["key"][:t] >> 7, np.repeat(np.arange(n, dtype=np.uint32), c)), what + ": ray ids of the keys"
    assert (g["key"][t:] == SENTINEL32).all() and (g["w"][t:] == SENTINEL32).all(), what + ": the unused tail was written"
    g["w"] = g["w"].view(F32)
    g["bins"], g["vals"] = SR.rows_of(g["off"], g["cnt"], g["key"], g["w"], n_max)
    return g


def same_rows(a, b, ids, what):
    """rows `ids` of result b are result a, bit for bit"""
    assert np.array_equal(a["cnt"], b["cnt"][ids]), what + ": counts"
    assert np.array_equal(a["bins"], b["bins"][ids]), what + ": bins"
    assert same_bits(a["vals"], b["vals"][ids]), what + ": kept values"


def _log(**ctx):
    return lambda s: record("selection_transform", **ctx, worst_residual=s["worst_residual"], bound=s["bound"], undecided=s["undecided"],
                            rays=s["rays"], thr=s["thr"])


@pytest.mark.parametrize("losses0", SR.LOSSES)
@pytest.mark.parametrize("kernel,n_max", KERNEL_N)
def test_selection_accuracy(ctxs, kernel, n_max, losses0):
    c = inputs(losses0)
    r = ctxs[losses0, kernel]
    raw = c["raw"]
    d_orc = r.to_device(raw)
    for thr in SR.thresholds(losses0):
        tag = "%s %s n_max %d thr %r" % (kernel, losses0, n_max, thr)
        g = run_compact(r, d_orc, raw.shape[0], n_max, thr, tag)
        SR.check_selection(raw, losses0, n_max, thr, g["cnt"], g["bins"], g["vals"], c["bound"], log=_log(kernel=kernel, losses0=losses0, n_max=n_max))
        SR.assert_edges(c, n_max, thr, g["cnt"], g["bins"], tag)
    d_orc.free()


@pytest.mark.parametrize("losses0", SR.LOSSES)
@pytest.mark.parametrize("kernel,n_max", POSITION_N)
def test_position_invariance(ctxs, kernel, n_max, losses0):
    c = inputs(losses0)
    r = ctxs[losses0, kernel]
    raw, thr = c["raw"], SR.THRESHOLDS[losses0]
    B = raw.shape[0]
    tag = "%s %s n_max %d" % (kernel, losses0, n_max)
    d_base = r.to_device(raw)
    base = run_compact(r, d_base, B, n_max, thr, tag + " base")
    SR.check_selection(raw, losses0, n_max, thr, base["cnt"], base["bins"], base["vals"], c["bound"])
    ids = permuted(LONG, B)
    assert np.unique(ids).size == B
    d_long = r.to_device(np.ascontiguousarray(raw[ids]))
    same_rows(run_compact(r, d_long, LONG, n_max, thr, tag + " long"), base, ids, tag + " %d rays" % LONG)
    for n in PREFIXES:
        same_rows(run_compact(r, d_long, n, n_max, thr, tag + " %d rays" % n), base, ids[:n], tag + " %d rays" % n)
    out = [Guarded(r, 4) for _ in range(5)]
    r.compact(d_long, 0, n_max, thr, *[g.ptr for g in out])
    r.sync()
    for g in out:
        assert (g.body(tag + " 0 rays") == 0xA5).all(), tag + ": zero rays wrote something"
    d_base.free()
    d_long.free()


@pytest.mark.parametrize("losses0", SR.LOSSES)
@pytest.mark.parametrize("n_max", PAIR_N)
def test_pair_against_wave(ctxs, n_max, losses0):
    c = inputs(losses0)
    raw = c["raw"]
    B = raw.shape[0]
    for thr in SR.thresholds(losses0):
        tag = "%s n_max %d thr %r" % (losses0, n_max, thr)
        res = {}
        for kernel in ("pair", "wave"):
            r = ctxs[losses0, kernel]
            d_orc = r.to_device(raw)
            res[kernel] = run_compact(r, d_orc, B, n_max, thr, tag + " " + kernel)
            d_orc.free()
        p, w = res["pair"], res["wave"]
        if losses0 not in SR.SOFTMAX:
            same_rows(p, w, np.arange(B), tag + " pair against wave")
            assert np.array_equal(p["key"], w["key"]) and np.array_equal(p["off"], w["off"]) and p["total"] == w["total"]
            continue
        compare_softmax(raw, losses0, n_max, thr, p, w, c["bound"], tag)


def compare_softmax(raw, losses0, n_max, thr, p, w, bound, tag):
    """what two selections whose softmax sums differ in order owe each other (d.)"""
    dec = None
    for name, g in (("pair", p), ("wave", w)):
        out = SR.check_selection(raw, losses0, n_max, thr, g["cnt"], g["bins"], g["vals"], bound)
        dec = out["decided"]      # a property of the inputs: the same for both
    same_set = (p["cnt"] == w["cnt"]) & (p["bins"] == w["bins"]).all(1)
    assert same_set[dec].all(), "%s: decided with margin, but pair and wave differ on rays %s" % (tag, np.flatnonzero(dec & ~same_set)[:8].tolist())
    a, b = p["vals"][same_set].astype(np.float64), w["vals"][same_set].astype(np.float64)
    with np.errstate(all="ignore"):
        far = np.abs(a - b) > bound * np.maximum(np.abs(a), np.abs(b)) + SR.FLOOR
    assert not (far & ~(np.isnan(a) & np.isnan(b))).any(), tag + ": kept values of pair and wave differ by more than the bound"
    record("selection_pair_against_wave", case=tag, rays=int(dec.size), undecided=int((~dec).sum()), different_sets=int((~same_set).sum()),
           different_values=int((a != b).sum()), bound=bound)
    return same_set


# ---- whole frames ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", TRANSFORM_CASES)
def test_fused_pair_and_wave_frames(name, tmp_path):
    z, meta, sc = load_case(name)
    d = str(tmp_path / "m")
    O.write_model_dir(d, sc, case_weights(meta))
    w, h = 97, 61
    n, n_max, thr = w * h, sc.num_samples, sc.threshold
    res, orc = {}, None
    for kind, kw in (("fused", {}), ("pair", dict(keep_oracle=True)), ("wave", dict(wave_select=True))):
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h), **kw) as r:
            r.set_camera(z["pose"], z["rot"])
            rgb, rgba, st = r.render_numpy()
            assert r.info.batch_rays >= n and st.sampling_overflow == 0
            g = dict(cnt=r.buffer(R.BUF_RAY_COUNTS, np.int32, (n,)), off=r.buffer(R.BUF_RAY_OFFSETS, np.int32, (n,)),
                     total=int(r.buffer(R.BUF_TOTAL, np.int32, (1,))[0]), rgb=rgb, rgba=rgba)
            g["key"], g["w"] = r.buffer(R.BUF_SAMPLE_KEY, np.uint32, (g["total"],)), r.buffer(R.BUF_SAMPLE_W, F32, (g["total"],))
            g["bins"], g["vals"] = SR.rows_of(g["off"], g["cnt"], g["key"], g["w"], n_max)
            if kind != "fused":      # both separate launches read the oracle buffer
                o = r.buffer(R.BUF_ORACLE, F32, (n, 128))
                assert orc is None or same_bits(o, orc), name + ": the raw outputs depend on the selection kernel"
                orc = o
            res[kind] = g
    bound = SR.transform_bound(orc, sc.losses0)
    for k in ("cnt", "off", "total", "key", "w", "rgb", "rgba"):      # both run pair_epilogue
        assert same_bits(np.asarray(res["fused"][k]), np.asarray(res["pair"][k])), "%s: %s of the fused and the pair selection differ" % (name, k)
    out = SR.check_selection(orc, sc.losses0, n_max, thr, res["pair"]["cnt"], res["pair"]["bins"], res["pair"]["vals"], bound,
                             log=_log(kernel="fused", losses0=sc.losses0, n_max=n_max, case=name))
    assert out["undecided"] <= 0.01 * n
    if sc.losses0 in SR.SOFTMAX:
        same_set = compare_softmax(orc, sc.losses0, n_max, thr, res["pair"], res["wave"], bound, name)
        if same_set.all():      # the kept values never reach compositing under these losses (mult_mode 0)
            assert same_bits(res["wave"]["rgba"], res["pair"]["rgba"]) and same_bits(res["wave"]["rgb"], res["pair"]["rgb"])
    else:
        for k in ("cnt", "off", "total", "key", "w", "rgb", "rgba"):
            assert same_bits(np.asarray(res["wave"][k]), np.asarray(res["pair"][k])), "%s: %s of the wave and the pair selection differ" % (name, k)


# ---- the budget trim --------------------------------------------------------------------------------------------------------------------

# n_max 32 runs in the wave context only: without ADANERF_FLAG_WAVE_SELECT a context selects n_max = 32 with select_kernel but the
# n_r <= 16 of the comparison with select_rows_kernel, and under the softmax the two owe each other d., not bits
@pytest.mark.parametrize("losses0", ["BCEWithLogitsLoss", "CrossEntropyLoss"])
@pytest.mark.parametrize("kernel,n_max", [("pair", 8), ("wave", 8), ("wave", 32)])
def test_budget_trim_under_a_transform(ctxs, kernel, n_max, losses0):
    c = inputs(losses0)
    r = ctxs[losses0, kernel]
    thr = SR.THRESHOLDS[losses0]
    n = 257
    ids = permuted(n, c["raw"].shape[0])
    raw = np.ascontiguousarray(c["raw"][ids])
    rng = np.random.default_rng(n_max)
    n_map = rng.choice(np.array([0, 1, 3, n_max // 2, n_max, n_max + 2], np.uint8), n)
    thr_map = rng.choice(np.array([0.5 * thr, thr, 1.5 * thr, 3.0 * thr], F32), n)
    n_eff = np.where((n_map == 0) | (n_map > n_max), n_max, n_map).astype(np.int64)
    thr_eff = np.where(thr_map > F32(thr), thr_map, F32(thr)).astype(F32)
    d_orc, d_n, d_t = r.to_device(raw), r.to_device(n_map), r.to_device(thr_map)
    tag = "%s %s n_max %d budget" % (kernel, losses0, n_max)
    got = run_compact(r, d_orc, n, n_max, thr, tag, maps=(d_n, d_t))
    assert len(set(zip(n_eff.tolist(), thr_eff.tolist()))) >= 10 and (got["cnt"] < n_max).any()
    for nr, tr in sorted(set(zip(n_eff.tolist(), thr_eff.tolist()))):
        rays = np.flatnonzero((n_eff == nr) & (thr_eff == F32(tr)))
        ref = run_compact(r, d_orc, n, int(nr), float(tr), tag + " reference (%d, %r)" % (nr, tr))
        assert np.array_equal(got["cnt"][rays], ref["cnt"][rays]), "%s: counts of the rays at (%d, %r)" % (tag, nr, tr)
        assert np.array_equal(got["bins"][rays, :nr], ref["bins"][rays]), "%s: bins of the rays at (%d, %r)" % (tag, nr, tr)
        assert (got["bins"][rays, nr:] == -1).all()
        assert same_bits(got["vals"][rays, :nr], ref["vals"][rays]), "%s: kept values of the rays at (%d, %r)" % (tag, nr, tr)
    for b in (d_orc, d_n, d_t):
        b.free()


# ---- dense mode ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("losses0", ["BCEWithLogitsLoss", "CrossEntropyLoss"])
def test_dense_mode_returns_the_raw_outputs(ctxs, losses0):
    """threshold 0 keeps every bin and ranks nothing: the weights are the network's outputs as they are, whatever losses[0] is"""
    raw = inputs(losses0)["raw"][:257]
    n = raw.shape[0]
    for kernel in ("pair", "wave"):
        r = ctxs[losses0, kernel]
        d_orc = r.to_device(raw)
        off, cnt, tot = Guarded(r, n * 4), Guarded(r, n * 4), Guarded(r, 4)
        key, w = Guarded(r, n * 128 * 4), Guarded(r, n * 128 * 4)
        r.compact(d_orc, n, 128, 0.0, off.ptr, cnt.ptr, key.ptr, w.ptr, tot.ptr)
        r.sync()
        assert int(tot.body("dense total", np.int32)[0]) == n * 128
        assert (cnt.body("dense counts", np.int32) == 128).all() and np.array_equal(off.body("dense offsets", np.int32), np.arange(n) * 128)
        assert np.array_equal(key.body("dense keys", np.uint32), np.arange(n * 128, dtype=np.uint32))
        assert same_bits(w.body("dense weights", F32), raw.reshape(-1)), losses0 + ": the dense mode's weights are not the raw outputs"
        d_orc.free()
