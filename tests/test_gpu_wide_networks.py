"""Hidden widths 257..512 on the device: the wide fp32 form (sampling nets wider than 256 in every sampling mode, fp32 shading, both nets
of coarse/fine mode) and the staged 16-bit shading kernel at width 512, against the reference's fixtures and the oracle."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import adanerf_oracle as O
from conftest import COARSE_FINE_CASES, case_weights, check_identical, load_case, record, residual_budget
from test_gpu_parity import model_dir, run_rows

import adanerf_amd

pytestmark = pytest.mark.gpu

WIDE_CASES = ["syn_w320_w512_skip4", "syn_w256_w384_skips_1_4"]


@pytest.mark.parametrize("name", WIDE_CASES)
def test_wide_networks_match_the_reference(name, tmp_path_factory):
    z, meta, sc = load_case(name)
    wts = case_weights(meta)
    d = model_dir(tmp_path_factory, sc, wts, "wide_" + name)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, meta["w"], meta["h"]), precision="bf16") as r:
        r.set_camera(z["pose"], z["rot"])
        assert r.info.n_in0 == sc.n_in0
        orc = run_rows(r, meta, lambda f, n, b: r.sample_mlp(f, n, b, None), 128)
        feat = run_rows(r, meta, lambda f, n, b: r.ray_features(f, n, b, None), sc.n_in0)
    n = z["oracle_in"].shape[0]
    np.testing.assert_allclose(feat[:n, :90], z["oracle_in"][:, :90], rtol=0, atol=2e-3)
    np.testing.assert_allclose(orc, z["oracle_out"], rtol=0, atol=3e-4)
    cnt, bins, _ = O.select_adaptive(orc, sc.num_samples, sc.threshold)
    same = (cnt == z["sel_count"]) & (bins == z["sel_bins"]).all(axis=1)
    check_identical(same, "wide_network_selection", 0, case=name)      # against the reference's own selection (fixture)
    # whole small frames against the oracle in every shading precision, batched and not
    w, h = 96, 64
    ref = O.render_rays(O.generate_ray_directions(w, h, sc.fov), z["pose"], z["rot"], sc, wts, w, h, keep=True)
    for prec, min_psnr in (("fp32", 90.0), ("fp16", 72.0), ("bf16", 50.0)):
        frames = []
        for bs in (-1, 2500):
            with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h, batch_size=bs), precision=prec) as r:
                r.set_camera(z["pose"], z["rot"])
                rgb, rgba, st = r.render_numpy()
                frames.append((rgb.copy(), rgba.copy(), int(st.total_samples)))
        assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1]), prec
        rgb, _, total = frames[0]
        if prec == "fp32":
            same = np.abs(rgb - ref["rgb"]).max(axis=1) < 3e-4
            check_identical(same, "wide_network_frame", residual_budget(w * h), case=name)
        p = O.psnr(rgb[same], ref["rgb"][same])
        record("wide_network_frame", case=name, prec=prec, psnr_db=p, max_abs=float(np.abs(rgb[same] - ref["rgb"][same]).max()),
               samples=total, ref_samples=int(ref["count"].sum()))
        assert p > min_psnr, (prec, p)
        assert abs(total - int(ref["count"].sum())) <= residual_budget(w * h) * sc.num_samples


def test_wide_sampling_nets_run_fp32_in_every_sampling_mode(tmp_path_factory):
    """A sampling net wider than 256 has no 16-bit packing: split, guarded, fp16 and fp32 requests all run the wide fp32 kernel."""
    z, meta, sc = load_case("syn_w320_w512_skip4")
    d = model_dir(tmp_path_factory, sc, case_weights(meta), "wide_modes")
    w, h = 96, 64
    frames = []
    for smp in ("split", "guarded", "fp16", "fp32"):
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h), precision="bf16", sampling=smp) as r:
            r.set_camera(z["pose"], z["rot"])
            rgb, rgba, st = r.render_numpy()
            frames.append((smp, rgb.copy(), rgba.copy()))
    for smp, rgb, rgba in frames[1:]:
        assert np.array_equal(rgb, frames[0][1]) and np.array_equal(rgba, frames[0][2]), smp


def test_wide_coarse_fine_frame_matches_the_oracle(tmp_path_factory):
    z, meta, sc = load_case(COARSE_FINE_CASES[0])
    sc = dataclasses.replace(sc, num_samples_coarse=16, num_samples=24)
    wts = O.synthetic_coarse_fine_weights(5, pos_enc=sc.pos_enc, alpha_bias=0.0, widths=(512, 512))
    d = model_dir(tmp_path_factory, sc, wts, "wide_cf")
    w, h = 72, 48
    ref = O.render_rays(O.generate_ray_directions(w, h, sc.fov), z["pose"], z["rot"], sc, wts, w, h)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h), precision="fp32") as r:
        r.set_camera(z["pose"], z["rot"])
        rgb, rgba, st = r.render_numpy()
    p = O.psnr(rgb, ref["rgb"])
    record("wide_coarse_fine_frame", psnr_db=p, max_abs=float(np.abs(rgb - ref["rgb"]).max()))
    assert p > 90.0, p


@pytest.mark.parametrize("seed", range(6))
def test_random_wide_topologies_match_the_oracle(seed, tmp_path_factory):
    rng = np.random.default_rng(900 + seed)
    z, meta, sc = load_case("syn_w320_w512_skip4")
    widths = (int(rng.integers(257, 513)), int(rng.integers(257, 513)))
    layers = (int(rng.integers(2, 9)), int(rng.integers(2, 9)))
    skips = sorted({int(s) for s in rng.integers(0, layers[1] - 1, size=int(rng.integers(0, 3)))}) if layers[1] > 1 else []
    wts = O.synthetic_weights(1000 + seed, n_in0=sc.n_in0, oracle_bias=0.1, oracle_scale=0.3, layers=layers, widths=widths,
                              skip1=skips if skips else 99)
    d = model_dir(tmp_path_factory, sc, wts, "wide_rand%d" % seed)
    w, h = 96, 64
    ref = O.render_rays(O.generate_ray_directions(w, h, sc.fov), z["pose"], z["rot"], sc, wts, w, h, keep=True)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h), precision="bf16") as r:
        r.set_camera(z["pose"], z["rot"])
        rgb, rgba, st = r.render_numpy()
        cnt = r.buffer(3, np.int32, (w * h,))
    same = cnt == ref["count"]
    check_identical(same, "wide_random_topology", residual_budget(w * h), seed=seed)
    p = O.psnr(rgb[same], ref["rgb"][same])
    record("wide_random_topology", seed=seed, layers=list(layers), widths=list(widths), skips=skips, psnr_db=p)
    assert p > 50.0, (layers, widths, skips, p)


def test_wide_context_returns_all_device_memory(tmp_path_factory):
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    z, meta, sc = load_case("syn_w320_w512_skip4")
    d = model_dir(tmp_path_factory, sc, case_weights(meta), "wide_life")

    def cycle():
        for prec in ("bf16", "fp16", "fp32"):
            with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 160, 120, batch_size=7000), precision=prec) as r:
                r.set_camera(z["pose"], z["rot"])
                r.render_numpy()

    cycle()
    base = free_bytes()
    for _ in range(3):
        cycle()
    assert abs(free_bytes() - base) <= 8 << 20, (base, free_bytes())


def test_wide_full_frame_is_finite(tmp_path_factory):
    """An 800 x 800 frame with an 8 x 512 bf16 shading net (the 16-bit staged kernel at width 512)."""
    z, meta, sc = load_case("syn_w320_w512_skip4")
    d = model_dir(tmp_path_factory, sc, case_weights(meta), "wide_800")
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 800, 800), precision="bf16") as r:
        r.set_camera(z["pose"], z["rot"])
        r.render_numpy()
        rgb, rgba, st = r.render_numpy()
    assert np.isfinite(rgb).all() and st.total_samples > 0
    record("wide_full_frame", w=800, h=800, samples=int(st.total_samples), ms_total=float(st.ms_total), ms_sample_mlp=float(st.ms_sample_mlp),
           ms_compact=float(st.ms_compact), ms_shade_mlp=float(st.ms_shade_mlp))
