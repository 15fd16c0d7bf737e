"""The comparators of tests/stage_reference.py can fail: the fp32 numpy oracle passes every one of them on the GPU tests' own inputs (and
its worst case, in the bounds' units, sits under half of every bound: the oracle-side constants next to stage_reference.C), and each of
thirteen emulated kernel faults, applied to an fp32 numpy emulation of the kernel, is refused.  The same for the depth and accumulation
maps: the emulations' worst case on the GPU tests' rows is what stage_reference.MEASURED_AUX states (the bound is twice it), and each of
four faults of the maps is refused."""
import dataclasses
import json
import os

import numpy as np
import pytest

import adanerf_oracle as O
import stage_reference as S
from conftest import load_case, record

import adanerf_amd
from adanerf_amd import renderer as R

COMPOSITE_N = {"thread": [1, 8, 9, 10, 19, 20, 32], "wave": [33, 64, 65, 127, 128]}
CLASSIC_N = {"classic_thread": [1, 2, 31, 32], "classic_wave": [33, 63, 64, 65, 128, 129, 192, 1024]}
PDF_N = [1, 2, 8, 63, 64, 65, 200]
PDF_MODELS = [("BCEWithLogitsLoss", "log"), ("BCEWithLogitsLoss", "linear"), ("CrossEntropyLoss", "log"), ("CrossEntropyLoss", "linear"),
              ("MSE", "log"), ("MSE", "linear")]
FINE_PAIRS = [(3, 1), (3, 8), (16, 24), (64, 128), (128, 1), (128, 128)]
MULTS = ["none", "alpha", "weights"]


def pdf_scene(losses0, depth_transform):
    z, meta, sc = load_case("synthetic_fixed8")
    return dataclasses.replace(sc, sampler="FromClassifiedDepth", losses0=losses0, depth_transform=depth_transform)


def fine_scene(nc, nf):
    z, meta, sc = load_case("classroom_coarse_fine_16_24")
    return dataclasses.replace(sc, num_samples_coarse=nc, num_samples=nf, depth_transform="linear")


def oracle_pdf_world(orc, n, sc):
    return O.to_world_depth(O.sample_pdf(orc, n, sc.losses0), sc)


def oracle_fine_rows(raw, zc, rays_d, nf):
    R = raw.shape[0]
    zcr = np.repeat(zc[None], R, 0)
    mid = (np.float32(0.5) * (zcr[:, 1:] + zcr[:, :-1])).astype(np.float32)
    zf = O.sample_pdf_bins(mid, O.classic_weights(raw, zcr, rays_d)[:, 1:-1], nf)
    return np.sort(np.concatenate([zcr, zf], -1), -1).astype(np.float32)


@pytest.fixture(scope="module")
def ztabs(tmp_path_factory):
    """The depth tables the GPU tests' contexts hold (bin centres; the dense mode's depths), from the host library"""
    adanerf_amd.build_library()
    lib = R.load_library()
    d = str(tmp_path_factory.mktemp("ztab"))
    O.write_model_dir(d, load_case("synthetic_fixed8")[2], O.synthetic_weights(1))
    zt = S.host_depth_table(lib, R._Options, d, 8, 0.2)
    assert np.array_equal(zt, S.host_depth_table(lib, R._Options, d, 100, 0.2))      # the bin centres do not depend on N
    dense = S.host_depth_table(lib, R._Options, d, 128, 0.0)
    assert np.isfinite(zt).all() and (np.diff(zt) > 0).all() and np.isfinite(dense).all() and not np.array_equal(zt, dense)
    return dict(adaptive=zt, dense=dense)


def adaptive_maps(c, mult, zt, key, kind, fault=None):
    """(units of depth, of acc) [R] of the emulation against fp64 on one layout; key None: the dense mode's bin = index & 127"""
    bins = (np.arange(c["raw"].shape[0]) if key is None else key) & 127
    _, rd, ra, scale = S.composite64(c["raw"], c["sw"], c["off"], c["cnt"], mult, z=zt[bins])
    _, d, a = S.composite32(c["raw"], c["sw"], c["off"], c["cnt"], mult, fault=fault, ztab=zt, key=key, order="seq" if kind == "thread" else "wave")
    return (d, a), (rd, ra), scale, S.ray_zmax(zt[bins], c["off"], c["cnt"])


def classic_maps(c, kind, fault=None):
    d3 = c["rays"][:, 4:7]
    _, rd, ra, scale = S.composite_classic64(c["raw"], c["z"], d3)
    _, d, a = S.composite_classic32(c["raw"], c["z"], d3, fault=fault, aux=True, order="seq" if kind == "classic_thread" else "wave")
    return (d, a), (rd, ra), scale, np.abs(c["z"].astype(np.float64)).max(1)


# ---- accept: the oracle passes, and its constants sit under the bounds -----------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(COMPOSITE_N))
def test_oracle_compositing_passes_and_sits_under_half_the_bound(kind):
    worst = 0.0
    for N in COMPOSITE_N[kind]:
        for mult in MULTS:
            c = S.composite_inputs(1000 + N, N)
            with np.errstate(all="ignore"):
                got = O.composite(c["raw"], c["sw"], c["off"], c["cnt"], mult if mult != "none" else "")
            ref, _, _, scale = S.composite64(c["raw"], c["sw"], c["off"], c["cnt"], mult)
            w = S.check_composite(got, ref, scale, c["cnt"], kind)
            assert np.array_equal(S.rgba8_of(got)[c["finite"]], O.to_rgba8(got)[c["finite"]])
            record("stage_oracle_composite", kernel=kind, N=N, mult=mult, worst_units=w)
            worst = max(worst, w)
    record("stage_oracle_composite_worst", kernel=kind, worst_units=worst, bound=S.C[kind])
    assert 2 * worst <= S.C[kind], (worst, S.C[kind])
    # the table states what is measured: the oracle-side figure to 10 % (numpy's exp differs a little between CPUs)
    m = S.MEASURED[kind]
    assert 0.9 * m["oracle"] <= worst <= 1.1 * m["oracle"], (worst, m)


@pytest.mark.parametrize("kind", list(CLASSIC_N))
def test_oracle_classic_compositing_passes_and_sits_under_half_the_bound(kind):
    worst = 0.0
    for n in CLASSIC_N[kind]:
        c = S.classic_inputs(2000 + n, n)
        with np.errstate(all="ignore"):
            got = O.composite_classic(c["raw"], c["z"], c["rays"][:, 4:7])
        ref, _, _, scale = S.composite_classic64(c["raw"], c["z"], c["rays"][:, 4:7])
        w = S.check_composite(got, ref, scale, n, kind)
        record("stage_oracle_classic", kernel=kind, n=n, worst_units=w)
        worst = max(worst, w)
    record("stage_oracle_classic_worst", kernel=kind, worst_units=worst, bound=S.C[kind])
    assert 2 * worst <= S.C[kind], (worst, S.C[kind])
    # the table states what is measured: the oracle-side figure to 10 % (numpy's exp differs a little between CPUs)
    m = S.MEASURED[kind]
    assert 0.9 * m["oracle"] <= worst <= 1.1 * m["oracle"], (worst, m)


@pytest.mark.parametrize("kind", list(COMPOSITE_N) + list(CLASSIC_N))
def test_map_emulations_pass_and_their_worst_case_is_half_the_bound(kind, ztabs):
    """MEASURED_AUX's emulation side, recomputed on the rows test_gpu_stage_kernels.py uses: the bound is exactly twice it"""
    worst = 0.0

    def one(K, ref, scale, zmax, count, **ctx):
        nonlocal worst
        wd, wa = S.check_aux(K[0], K[1], ref[0], ref[1], scale, zmax, count, kind)
        record("stage_emulation_aux", kernel=kind, worst_units_depth=wd, worst_units_acc=wa, **ctx)
        worst = max(worst, wd, wa)
    if kind in COMPOSITE_N:
        for N in COMPOSITE_N[kind]:
            c = S.composite_inputs(1000 + N, N)
            idx = np.arange(c["key"].shape[0])
            assert ((c["key"] & 127) != (idx & 127)).mean() > 0.5 or N == 1        # a lookup by index is another depth
            for r in range(c["cnt"].shape[0]):                                       # ascending, distinct bins: the compactor's order
                assert (np.diff((c["key"][c["off"][r]:c["off"][r] + c["cnt"][r]] & 127).astype(np.int64)) > 0).all()
            for mult in MULTS:
                one(*adaptive_maps(c, mult, ztabs["adaptive"], c["key"], kind), c["cnt"], N=N, mult=mult)
        if kind == "wave":
            c = S.dense_layout()
            one(*adaptive_maps(c, "alpha", ztabs["dense"], None, kind), c["cnt"], N=128, mult="alpha", case="dense128")
    else:
        for n in CLASSIC_N[kind]:
            one(*classic_maps(S.classic_inputs(2000 + n, n), kind), n, n=n)
    record("stage_emulation_aux_worst", kernel=kind, worst_units=worst, bound=S.C_AUX[kind])
    m = S.MEASURED_AUX[kind]
    assert S.C_AUX[kind] == 2 * m["emulation"] and 2 * worst <= S.C_AUX[kind]
    # the table states what is measured, to 10 % (numpy's exp differs a little between CPUs)
    assert 0.9 * m["emulation"] <= worst <= 1.1 * m["emulation"], (worst, m)


def test_bounds_are_twice_the_larger_worst_case_of_the_committed_log():
    """stage_reference.MEASURED against profiles/stage_kernels_measured.log: per kernel family the largest worst_units of the oracle's
    lines (this suite) and of the kernels' lines (test_gpu_stage_kernels.py on an MI355X), each rounded up to 1e-4; the log has a
    kernel-side line for every case of the dispatch table"""
    lines = [json.loads(l) for l in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "stage_kernels_measured.log"))]
    sizes = {**COMPOSITE_N, **CLASSIC_N}
    for kind, m in S.MEASURED.items():
        side = {"oracle": [l for l in lines if l["test"] in ("stage_oracle_composite", "stage_oracle_classic") and l["kernel"] == kind],
                "device": [l for l in lines if l["test"] == "stage_kernel" and l["kernel"] == kind]}
        for name, ls in side.items():
            worst = max(l["worst_units"] for l in ls)
            assert worst <= m[name] < worst + 1e-4, (kind, name, worst, m[name])
            assert {l.get("N", l.get("n")) for l in ls} == set(sizes[kind]), (kind, name)
        assert all(l["non_finite_rule"] and l["bound"] == S.C[kind] for l in side["device"])
        assert S.C[kind] == 2 * max(m["oracle"], m["device"])
    # the maps: the emulation's lines (this suite) make the bound, the kernels' lines (an MI355X) are stated and lie under it
    for kind, m in S.MEASURED_AUX.items():
        emu = [l for l in lines if l["test"] == "stage_emulation_aux" and l["kernel"] == kind]
        dev = [l for l in lines if l["test"] == "stage_kernel_aux" and l["kernel"] == kind]
        worst = max(max(l["worst_units_depth"], l["worst_units_acc"]) for l in emu)
        assert worst <= m["emulation"] < worst + 1e-4, (kind, worst, m)
        assert S.C_AUX[kind] == 2 * m["emulation"]
        worst = max(l["worst_units"] for l in dev)
        assert worst <= m["device"] < worst + 1e-4, (kind, worst, m)
        for ls in (emu, dev):
            assert {l.get("N", l.get("n")) for l in ls} == set(sizes[kind]), kind
        assert {l["map"] for l in dev} == {"depth", "acc"}
        assert all(l["non_finite_rule"] and l["bound"] == S.C_AUX[kind] and l["worst_units"] <= l["bound"] for l in dev), kind
        if kind in COMPOSITE_N:
            assert {l["mult"] for l in dev} == set(MULTS) == {l["mult"] for l in emu}
        if kind == "wave":
            assert any(l.get("case") == "dense128" for l in emu) and any(l.get("case") == "dense128" for l in dev)
    dev = [l for l in lines if l["test"] == "stage_kernel"]
    assert {l["n"] for l in dev if l["kernel"] == "pdf_sample_kernel"} == set(PDF_N)
    assert len([l for l in dev if l["kernel"] == "pdf_sample_kernel"]) == len(PDF_N) * len(PDF_MODELS)
    assert {(l["nc"], l["nf"]) for l in dev if l["kernel"] == "fine_sample_kernel"} == set(FINE_PAIRS)
    assert all(l["worst_residual"] <= l["bound"] == 2 * l["oracle_residual"] for l in dev if "worst_residual" in l)


@pytest.mark.parametrize("losses0,dt", PDF_MODELS)
def test_oracle_pdf_sampler_residual(losses0, dt):
    sc = pdf_scene(losses0, dt)
    orc, fin = S.pdf_rows(3000, losses0, nonfinite=False)
    for n in PDF_N:
        zw = oracle_pdf_world(orc, n, sc)
        res, _ = S.pdf_residual(zw, orc, n, losses0, sc.depth_range, dt == "log")
        b = S.sampler_bound(res)
        record("stage_oracle_pdf", losses0=losses0, depth=dt, n=n, worst_residual=b / 2)
        # by construction: the denom < 1e-5 fall-back (1e-5) + fp32 noise of the scan and of the depth written in fp32
        assert b / 2 < 4e-5, (n, b / 2)
        R = orc.shape[0]
        bins = np.clip(np.floor(S.from_world64(zw, sc.depth_range, dt == "log") * 128), 0, 127).astype(np.uint32)
        key = (np.arange(R, dtype=np.uint32)[:, None] << 7) | bins
        S.check_pdf(zw, key, np.zeros(R * n, np.float32), np.arange(R) * n, np.full(R, n, np.int32), R * n, orc, n, losses0, sc.depth_range,
                    dt == "log", b)


@pytest.mark.parametrize("nc,nf", FINE_PAIRS)
def test_oracle_fine_sampler_residual(nc, nf):
    sc = fine_scene(nc, nf)
    zc = O.coarse_depths(sc)
    c = S.fine_inputs(4000 + nc, nc, nonfinite=False)
    rows = oracle_fine_rows(c["raw"], zc, c["rays"][:, 4:7], nf)
    res = S.fine_residual(S.split_fine_rows(rows, zc, nf), c["raw"], zc, c["rays"][:, 4:7], nf)
    b = S.sampler_bound(res)
    record("stage_oracle_fine", nc=nc, nf=nf, worst_residual=b / 2)
    # by construction: the denom < 1e-5 fall-back + the fp32 rounding of alpha = 1 - exp(-x) (an ulp of 1) against the smallest pdf
    # denominator there is, (nc - 2) 1e-5 on a ray through empty space
    assert b / 2 < 1e-5 + 8 * 2.0 ** -24 / ((nc - 2) * 1e-5), b / 2
    S.check_fine(rows, c["raw"], zc, c["rays"][:, 4:7], nf, b)


# ---- reject: the emulations pass without a fault, and every fault is refused -------------------------------------------------------------------

def refused(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("fault,N,mult", [("inclusive", 40, "alpha"), ("no_half_total", 100, "alpha"), ("no_half_total", 128, "none"),
                                          ("mult2_on_alpha", 100, "weights"), ("mult2_on_alpha", 16, "weights")])
def test_compositing_faults_are_refused(fault, N, mult):
    c = S.composite_inputs(1000 + N, N)
    ref, _, _, scale = S.composite64(c["raw"], c["sw"], c["off"], c["cnt"], mult)
    kind = "wave" if N > 32 else "thread"
    S.check_composite(S.composite32(c["raw"], c["sw"], c["off"], c["cnt"], mult), ref, scale, c["cnt"], kind)
    bad = S.composite32(c["raw"], c["sw"], c["off"], c["cnt"], mult, fault=fault)
    assert refused(lambda: S.check_composite(bad, ref, scale, c["cnt"], kind))


@pytest.mark.parametrize("fault,n", [("no_lap_carry", 65), ("no_lap_carry", 192), ("last_zero", 40), ("last_zero", 8), ("no_relu", 128), ("no_relu", 16)])
def test_classic_compositing_faults_are_refused(fault, n):
    c = S.classic_inputs(2000 + n, n)
    d = c["rays"][:, 4:7]
    ref, _, _, scale = S.composite_classic64(c["raw"], c["z"], d)
    kind = "classic_wave" if n > 32 else "classic_thread"
    S.check_composite(S.composite_classic32(c["raw"], c["z"], d), ref, scale, n, kind)
    bad = S.composite_classic32(c["raw"], c["z"], d, fault=fault)
    assert refused(lambda: S.check_composite(bad, ref, scale, n, kind))


@pytest.mark.parametrize("fault,N,mult", [("z_by_index", 8, "alpha"), ("z_by_index", 19, "none"), ("z_by_index", 33, "weights"), ("z_by_index", 127, "alpha"),
                                          ("aux_without_mult", 8, "weights"), ("aux_without_mult", 32, "weights"), ("aux_without_mult", 65, "weights"),
                                          ("aux_without_mult", 128, "weights"), ("aux_second_half_unmasked", 65, "none"),
                                          ("aux_second_half_unmasked", 127, "alpha"), ("aux_second_half_unmasked", 128, "weights")])
def test_map_faults_are_refused(fault, N, mult, ztabs):
    kind = "wave" if N > 32 else "thread"
    c = S.composite_inputs(1000 + N, N)
    K, ref, scale, zmax = adaptive_maps(c, mult, ztabs["adaptive"], c["key"], kind)
    wd, wa = S.check_aux(K[0], K[1], ref[0], ref[1], scale, zmax, c["cnt"], kind)
    assert 2 * max(wd, wa) <= S.C_AUX[kind]
    bad = adaptive_maps(c, mult, ztabs["adaptive"], c["key"], kind, fault=fault)[0]
    assert refused(lambda: S.check_aux(bad[0], None, ref[0], None, scale, zmax, c["cnt"], kind))      # the depth map refuses every one
    if fault != "z_by_index":                                                                             # acc does not see the table
        assert refused(lambda: S.check_aux(None, bad[1], None, ref[1], scale, zmax, c["cnt"], kind))
    # the faults are finite errors on finite rays, not only a NaN read from a neighbour
    fin = c["finite"] & (c["cnt"] > 0)
    u, _ = S.composite_units(bad[0][fin], ref[0][fin], (scale * zmax)[fin], c["cnt"][fin])
    assert np.nanmax(np.where(np.isfinite(u), u, 0.0)) > S.C_AUX[kind]


@pytest.mark.parametrize("n", [2, 32, 65, 129, 1024])
def test_classic_depth_fault_is_refused(n):
    kind = "classic_wave" if n > 32 else "classic_thread"
    c = S.classic_inputs(2000 + n, n)
    K, ref, scale, zmax = classic_maps(c, kind)
    wd, wa = S.check_aux(K[0], K[1], ref[0], ref[1], scale, zmax, n, kind)
    assert 2 * max(wd, wa) <= S.C_AUX[kind]
    bad = classic_maps(c, kind, fault="classic_depth_next_z")[0]
    assert refused(lambda: S.check_aux(bad[0], None, ref[0], None, scale, zmax, n, kind))
    assert same_or_nan(bad[1], K[1])


def same_or_nan(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("fault,n", [("no_eps", 65), ("u_k_over_n", 8), ("u_k_over_n", 200), ("no_lower_total", 64)])
def test_pdf_sampler_faults_are_refused(fault, n):
    losses0, dt = "BCEWithLogitsLoss", "log"
    sc = pdf_scene(losses0, dt)
    orc, fin = S.pdf_rows(3000, losses0, nonfinite=False)
    R = orc.shape[0]
    res, _ = S.pdf_residual(oracle_pdf_world(orc, n, sc), orc, n, losses0, sc.depth_range, True)
    b = S.sampler_bound(res)

    def check(t):
        zw = O.to_world_depth(t, sc)
        bins = np.clip(np.floor(S.from_world64(zw, sc.depth_range, True) * 128), 0, 127).astype(np.uint32)
        key = (np.arange(R, dtype=np.uint32)[:, None] << 7) | bins
        S.check_pdf(zw, key, np.zeros(R * n, np.float32), np.arange(R) * n, np.full(R, n, np.int32), R * n, orc, n, losses0, sc.depth_range, True, b)
    check(S.pdf32(orc, n, losses0))
    assert refused(lambda: check(S.pdf32(orc, n, losses0, fault=fault)))


@pytest.mark.parametrize("fault,nc,nf", [("w0_in_pdf", 16, 24), ("w0_in_pdf", 64, 128), ("drop_coarse", 16, 24), ("drop_coarse", 128, 1),
                                         ("dup_coarse", 16, 24), ("dup_coarse", 64, 128)])
def test_fine_sampler_faults_are_refused(fault, nc, nf):
    sc = fine_scene(nc, nf)
    zc = O.coarse_depths(sc)
    c = S.fine_inputs(4000 + nc, nc, nonfinite=False)
    d = c["rays"][:, 4:7]
    rows = oracle_fine_rows(c["raw"], zc, d, nf)
    b = S.sampler_bound(S.fine_residual(S.split_fine_rows(rows, zc, nf), c["raw"], zc, d, nf))
    S.check_fine(S.fine32(c["raw"], zc, d, nf), c["raw"], zc, d, nf, b)
    assert refused(lambda: S.check_fine(S.fine32(c["raw"], zc, d, nf, fault=fault), c["raw"], zc, d, nf, b))


def test_rgba8_rounding_fault_is_refused():
    rng = np.random.default_rng(5)
    rgb = np.concatenate([rng.uniform(-0.5, 1.8, (4096, 3)), [[np.nan, -0.0, 1.0], [np.inf, -np.inf, 0.999999], [0.5 / 255, 254.5 / 255, 1.0000001]]]).astype(np.float32)
    ok = S.rgba8_of(rgb)
    assert (ok[:, 3] == 255).all() and ok[-3].tolist() == [0, 0, 255, 255] and ok[-2].tolist()[:2] == [255, 0]
    fin = np.isfinite(rgb).all(1)
    assert np.array_equal(ok[fin], O.to_rgba8(rgb[fin]))
    assert not np.array_equal(S.rgba8_of(rgb, fault="round"), ok)
