"""The exact-by-construction sampling networks of tests/tie_networks.py, CPU side: what tests/test_gpu_fused_selection_edges.py relies on
is shown here, on the oracle's features of the 97 x 61 frame, for every model that file uses --

 a. the predicted rows equal mlp_reference.sampling_mlp64 on every saturated ray under each rounding model (exact, fp16, split), with exact
    accumulation and with fp32 products summed in another order (f32=True): equality, no tolerance;
 b. the class floors (tie_networks.FLOORS) on that frame: conditions on the construction, not measurements;
 c. adanerf_host_pack_weights takes every model in the forms its engines need: a refused model fails here, not on the GPU;
 d. O.select_adaptive keeps the lowest bins among ties on the predicted rows: against a three-line brute force, which pins the reference
    rule itself on these rows."""
import ctypes as C

import numpy as np
import pytest

import adanerf_oracle as O
import mlp_reference as M
import tie_networks as T
from conftest import load_case
from mfma_emulation import pack_weights

import adanerf_amd
from adanerf_amd import renderer as R

PACK_SPLIT = 3      # adanerf_host_pack_weights: the sampling net's fp16 hi / lo' pairs


@pytest.fixture(scope="module")
def base_case():
    return load_case("synthetic_fixed8")


@pytest.fixture(scope="module")
def built(base_case):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = T.build(name, base_case)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(T.MODELS))
def test_predicted_rows_equal_every_rounding_model(built, name):
    sc, wts, gates, feat = built(name)
    bins = gates["bins"]
    sat, rows = T.predict(feat, gates)
    sat16, rows16 = T.predict(feat, gates, engine16=True)
    over = T.overflow_open(feat, gates) & sat
    assert (over.mean() > T.FLOORS["tie"]) == T.MODELS[name]["overflow"]
    for model in ("exact", "fp16", "split"):
        for f32 in (False, True):
            with np.errstate(over="ignore", invalid="ignore"):
                y = T.pad_rows(M.sampling_mlp64(feat, wts.net0, model, f32=f32), np.float64)
            if model == "exact":
                assert np.array_equal(y[sat], rows[sat]), (name, model, f32)
                assert np.isfinite(y).all()
            else:      # operands in fp16: the row is not finite where the overflow gate is open, and the prediction elsewhere
                assert np.array_equal(y[sat & ~over], rows[sat & ~over]), (name, model, f32)
                assert not np.isfinite(y[over]).any(axis=1).any() if model == "fp16" else not np.isfinite(y[over]).all(axis=1).any(), (name, model, f32)
                assert np.isnan(rows16[over]).all() and np.array_equal(rows16[sat & ~over], rows[sat & ~over])
    # fp16 holds every predicted value, so the device's fp32 rows are these numbers bit for bit
    fin = rows[sat][:, :bins]
    assert np.array_equal(fin.astype(np.float16).astype(np.float64), fin) and np.array_equal(fin * 8, np.round(fin * 8))


@pytest.mark.parametrize("name", T.PLAIN)
def test_class_floors(built, name):
    sc, wts, gates, feat = built(name)
    sat, rows = T.predict(feat, gates)
    # the rows of all rays, transition bands included, as a correct split engine returns them
    y = T.pad_rows(M.sampling_mlp64(feat, wts.net0, "split", f32=True))
    assert np.array_equal(y[sat].astype(np.float64), rows[sat])
    assert sat.mean() >= T.FLOORS["saturated"], sat.mean()
    assert len(np.unique(rows[sat], axis=0)) >= T.FLOORS["distinct"]
    T.check_floors({(n, thr, kind): T.class_counts(y, sat, n, thr) for n, thr, kind in T.WALK}, name)


@pytest.mark.parametrize("name", T.OVERFLOW)
def test_overflow_models_keep_ties_beside_the_non_finite_rays(built, name):
    sc, wts, gates, feat = built(name)
    sat, rows = T.predict(feat, gates)
    over = T.overflow_open(feat, gates) & sat
    assert T.FLOORS["tie"] < over.mean() < 0.6, over.mean()
    assert T.mixed_blocks(over) >= T.FLOORS["tie_blocks"]
    c = T.classes(np.where(np.isnan(rows), 0, rows).astype(np.float32), 8, 0.125)
    assert (c["tie"] & sat & ~over).mean() >= T.FLOORS["tie"]
    # the rule's reading of a non-finite row: NaN never ranks, an all-NaN row keeps bin 0 with its own value
    nan_rows = np.full((3, 128), np.nan, np.float32)
    nan_rows[1, 77] = -3.0
    nan_rows[2, [5, 9]] = np.inf
    cnt, b, w = O.select_adaptive(nan_rows, 8, 0.125)
    assert cnt.tolist() == [1, 1, 2] and b[0, 0] == 0 and b[1, 0] == 77 and b[2, :2].tolist() == [5, 9] and np.isnan(w[0, 0])


@pytest.mark.parametrize("name", list(T.MODELS))
def test_packer_accepts_the_model(built, name, tmp_path):
    sc, wts, gates, feat = built(name)
    d = str(tmp_path / name)
    O.write_model_dir(d, sc, wts)
    adanerf_amd.build_library()
    lib = R.load_library()
    fixed = name.startswith("fixed")
    for prec in ([R.PREC_FP16] if fixed else []) + [PACK_SPLIT, R.PREC_FP32]:
        w, b, lay = pack_weights(lib, d, 0, prec)
        assert lay.shape[0] >= T.MODELS[name]["depth"] and w.size > 0 and np.isfinite(b).all()
    # the parse the device context makes: the shape the kernels are chosen by
    f = lib.adanerf_host_parse_model
    f.argtypes, f.restype = [C.c_char_p, C.c_void_p, C.POINTER(R.Info)], C.c_int
    opt = R._Options(width=T.W, height=T.H, batch_rays=-1, num_samples=0, threshold=-1.0, shard_world=1, strip_rows=8)
    info = R.Info()
    assert f(d.encode(), C.byref(opt), C.byref(info)) == 0, lib.adanerf_last_error(None)
    assert info.n_in0 == sc.n_in0 and info.rays_local == T.W * T.H


@pytest.mark.parametrize("name", T.PLAIN)
def test_reference_rule_on_the_predicted_rows(built, name):
    sc, wts, gates, feat = built(name)
    sat, rows = T.predict(feat, gates)
    uniq = np.unique(rows[sat], axis=0).astype(np.float32)
    ties = 0
    for n, thr, kind in T.WALK:
        cnt, b, w = O.select_adaptive(uniq, n, thr)
        tie = T.classes(uniq, n, thr)
        for i, row in enumerate(uniq):
            want = T.brute_force_select(row.tolist(), n, thr)
            assert b[i, :cnt[i]].tolist() == want and (b[i, cnt[i]:] == -1).all(), (name, n, thr, i)
            assert w[i, :cnt[i]].tolist() == [row[k] for k in want]
            if tie["tie"][i] or tie["max_tie"][i]:      # "lower bin first": a tied bin that was left out lies above every kept bin of its value
                ties += 1
                cut = min(row[k] for k in want)
                out = [k for k in range(128) if row[k] == cut and k not in want]
                assert out and min(out) > max(k for k in want if row[k] == cut)
    assert ties >= len(T.WALK)
