"""The 16-bit sampling engines at the edges of their operand range, bit for bit: range probes (tests/range_networks.py; its CPU side is
tests/test_sampling_ranges_cpu.py) are networks in which every matrix sum has one non-zero term, so what adanerf_sample_mlp returns is the
engine's operand rounding of a chosen constant or of gain x identity column, and nothing else -- fp16 subnormal hi, hi = 0 with lo'
carrying, subnormal lo', ties in either conversion, weights whose hi part is subnormal or zero, the last finite values below 65520, and
activations that cross 65520 inside the frame.  Frame 97 x 61 (5 917 rays: 47 tiles of 128, the last ragged); inputs are the device's own
adanerf_ray_features rows; one model directory and one small context per probe and engine.

Kernels and the cases that reach them (filed under the kernel that ran, as test_gpu_fused_encodings.py does):
  sample_mlp16x3_kernel <10, 4 | 2, 2>                         test_range_probes / test_range_edges [fixed_10_4], [fixed_2_2]  mode split
  sample_mlp16_kernel <10, 4 | 2, 2>                           the same cases, mode fp16 under $ADANERF_DEBUG_GUARD = 2
  sample_mlp16x2_kernel <10, 4 | 2, 2>                         test_two_block_kernel_on_range_probes: fused frames under = 4 against = 2
  sample_mlp16x3_gen_kernel <10, 4, W = 64 | 128 | 256>        [gen_w64_d4], [gen_w128_d5], [gen_w256_d6]  mode split
  sample_mlp_kernel / sample_mlp_gen_kernel / _gen_wide_kernel the same cases and [wide_w384_d4], mode fp32: the fp32 bits (control)

Every comparison is an equality, or the one-rounding bracket of range_networks.bracket where the cross term Whi xlo' + Wlo' xhi has two
non-zero products (the form of that one rounding inside the matrix pipe is not documented); on every ray and every column, none left out.
A ray the prediction calls BAD (an operand >= 65520, inf or NaN) must come back non-finite in EVERY column, and
adanerf_stats.sampling_overflow of one frame of a fresh context must equal the number of such rays (fp32: 0).  The only free numbers are the
class floors (range_networks.FLOORS), met by the oracle's features on the CPU and asserted here on the device's own rows.

What the probes hold, per case:
  table              the constants table below the top of the range, -0.0, every value negated, gains on known values      finite everywhere
  rays               every gain on every identity column it keeps in range                                                  finite everywhere
  top_split          32768, 65504, 65512, 65520 - 2^-7                                                          finite everywhere, counter 0
  top                32768, 65504, 65512, nextafter(65520, 0): finite with counter 0 in plain fp16 and fp32.  In the split engine the last
                     entry is carried as hi = 65504, lo' = 32768 -- the value 65520 -- and overflows at the next hidden layer: BAD on every
                     ray, counter 5 917 (the rule's own answer: test_sampling_ranges_cpu.py::test_the_table_entry_beyond_the_split_range;
                     include/adanerf_hip.h states it)
  overflow           65520, 1e5, 3e38, +inf, a NaN bias: BAD on every ray in every engine (0 x inf = NaN in fp32 as well), 16-bit counter 5 917
  overflow_finite32  65520, 1e5, 3e38: BAD in the 16-bit engines; the fp32 engine returns the three values' bits, counter 0
  edge0, edge1       2^15 f x m crossing 65520 inside the frame, beside the constants around 1: the rays beyond the edge BAD and counted,
                     every other ray exact -- the 1 % band test_sampling_fp16_range_contract leaves out
A weight outside the fp16 range (test_weight_outside_the_fp16_range): adanerf_create refuses it for the 16-bit engines and runs it in fp32.
Position invariance: the table probe from test_gpu_fused_encodings.WINDOWS returns the whole-frame bits, per engine.  Outputs sit between
4 KiB canaries (Guarded).  Figures: profiles/sampling_ranges_measured.md."""
import dataclasses
import time

import numpy as np
import pytest

import adanerf_oracle as O
import range_networks as RN
import tie_networks as T
from conftest import load_case, record
from test_gpu_fused_encodings import WINDOWS, device_rays
from test_gpu_fused_selection_edges import Live, rule, same
from test_gpu_mlp_engines import Guarded

import adanerf_amd

pytestmark = pytest.mark.gpu

W, H, N_RAYS = RN.W, RN.H, RN.W * RN.H
# id: depth, width, posEncArgs[0], sampling modes.  Run-time-shaped networks have no plain-fp16 engine; widths above 256 run the fp32 kernel alone
CASES = {
    "fixed_10_4": (8, 256, (10, 4), ("split", "fp16", "fp32")),
    "fixed_2_2": (8, 256, (2, 2), ("split", "fp16", "fp32")),
    "gen_w64_d4": (4, 64, (10, 4), ("split", "fp32")),
    "gen_w128_d5": (5, 128, (10, 4), ("split", "fp32")),
    "gen_w256_d6": (6, 256, (10, 4), ("split", "fp32")),
    "wide_w384_d4": (4, 384, (10, 4), ("fp32",)),
}


def kernel_of(case, mode):
    fixed = case.startswith("fixed")
    if mode == "fp32":
        return "sample_mlp_kernel" if fixed else ("sample_mlp_gen_wide_kernel" if case.startswith("wide") else "sample_mlp_gen_kernel")
    return ("sample_mlp16x3_kernel" if mode == "split" else "sample_mlp16_kernel") if fixed else "sample_mlp16x3_gen_kernel"


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def base_case():
    return load_case("synthetic_fixed8")


@pytest.fixture(scope="module")
def filler():
    return O.synthetic_weights(1).net1


def context(d, mode, z, monkeypatch):
    """a small context on the model directory d; plain fp16 runs the 8-wave kernel ($ADANERF_DEBUG_GUARD = 2, read at create)"""
    if mode == "fp16":
        monkeypatch.setenv("ADANERF_DEBUG_GUARD", "2")
    else:
        monkeypatch.delenv("ADANERF_DEBUG_GUARD", raising=False)
    r = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), precision="bf16", sampling=mode)
    r.init()
    r.set_camera(z["pose"], z["rot"])
    return r


@pytest.fixture(scope="module")
def scenes(base_case, filler, tmp_path_factory):
    """case -> (scene, the device's own feature rows of the frame, read-only): once per case"""
    cache = {}

    def get(case):
        if case not in cache:
            depth, width, pe0, modes = CASES[case]
            z, meta, sc0 = base_case
            sc = dataclasses.replace(sc0, pos_enc=(tuple(pe0), sc0.pos_enc[1]))
            d = str(tmp_path_factory.mktemp("range_feat_" + case))
            O.write_model_dir(d, sc, O.Weights(RN.range_probe(sc.n_in0, depth, width, RN.const_entries(RN.AROUND_ONE))[0], filler))
            with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), precision="bf16", sampling="fp32") as r:
                r.set_camera(z["pose"], z["rot"])
                assert r.info.n_in0 == sc.n_in0
                feat = device_rays(r, sc)[3]
            feat.setflags(write=False)
            cache[case] = (sc, feat)
        return cache[case]
    return get


def stage_rows(r, what):
    out = Guarded(r, N_RAYS * 512)
    r.sample_mlp(0, N_RAYS, out.ptr, None)
    r.sync()
    rows = out.body(what).view(np.float32).reshape(N_RAYS, 128).copy()
    out.free()
    return rows


def check_rows(rows, feat, chains, mode, what, names):
    """every ray and column of a probe's rows against the prediction -> range_networks.compare's counts"""
    k = len(chains)
    lo, hi, rne, bad = RN.bracket(feat, chains, mode)
    c = RN.compare(rows[:, :k], lo, hi, rne, bad)
    cols = np.flatnonzero(c["wrong"].any(axis=0))
    first = {names[j]: (int(np.flatnonzero(c["wrong"][:, j])[0]), int(c["wrong"][:, j].sum())) for j in cols[:8]}
    detail = {n: (ray, cnt, float(rows[ray, names.index(n)]), float(lo[ray, names.index(n)]), float(hi[ray, names.index(n)]), bool(bad[ray]))
              for n, (ray, cnt) in first.items()}
    assert not c["wrong"].any(), "%s: entries outside the prediction, name: (first ray, rays, got, lower, upper, ray is BAD) %s" % (what, detail)
    assert not rows[~bad][:, k:].any(), what + ": an output without an entry is not +0 on a ray inside the range"
    assert not np.isfinite(rows[bad]).any(), what + ": a ray beyond the range has a finite column"
    return c, bad


def log_figures(case, mode, name, c, seconds=None):
    record("sampling_ranges", case=case, kernel=kernel_of(case, mode), mode=mode, probe=name, **{k: v for k, v in c.items() if k != "wrong"},
           **({} if seconds is None else dict(seconds=seconds)))


def add(total, c):
    for k, v in c.items():
        if k != "wrong":
            total[k] = total.get(k, 0) + v
    return total


# ---- inside the range: the table and the ray-driven rows ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_range_probes(case, scenes, base_case, filler, tmp_path_factory, monkeypatch):
    depth, width, pe0, modes = CASES[case]
    z = base_case[0]
    sc, feat = scenes(case)
    dc, pc = T.identity_columns(sc)
    sets = dict(table=RN.table_entries(), rays=RN.ray_entries(dc, pc, feat))
    flags = []
    for name, entries in sets.items():
        for ci, ent in enumerate(RN.chunks(entries, width)):
            net, chains = RN.range_probe(sc.n_in0, depth, width, ent, seed=ci)
            names = [n for n, _ in ent]
            if name == "rays":
                flags.append(RN.class_flags(feat, chains))
            d = str(tmp_path_factory.mktemp("range_%s_%s_%d" % (case, name, ci)))
            O.write_model_dir(d, sc, O.Weights(net, filler))
            for mode in modes:
                t0 = time.perf_counter()
                r = context(d, mode, z, monkeypatch)
                try:
                    rows = stage_rows(r, "%s %s %s" % (case, name, mode))
                    c, bad = check_rows(rows, feat, chains, mode, "%s %s[%d] %s" % (case, name, ci, mode), names)
                    assert not bad.any(), "%s %s %s: the prediction sends a ray out of range" % (case, name, mode)
                    if name == "table":      # constant units: every ray returns the same row
                        assert (RN.bits(rows) == RN.bits(rows[:1])).all(), "%s table %s: rows differ between rays" % (case, mode)
                        if ci == 0:          # position invariance
                            for first, n in WINDOWS:
                                win = Guarded(r, n * 512)
                                r.sample_mlp(first, n, win.ptr, None)
                                r.sync()
                                got = win.body("window (%d, %d)" % (first, n)).view(np.float32).reshape(n, 128)
                                assert got.tobytes() == rows[first:first + n].tobytes(), "%s %s: rays (%d, %d) differ from the whole-frame call" % (case, mode, first, n)
                                win.free()
                finally:
                    r.close()
                log_figures(case, mode, "%s[%d]" % (name, ci), c, time.perf_counter() - t0)
    shares = RN.class_shares(flags)
    record("sampling_ranges_classes", case=case, **shares)
    RN.check_floors(shares, case + ": the device's own rows")


# ---- at and beyond the edge ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_range_edges(case, scenes, base_case, filler, tmp_path_factory, monkeypatch):
    depth, width, pe0, modes = CASES[case]
    z = base_case[0]
    sc, feat = scenes(case)
    dc, pc = T.identity_columns(sc)
    sets = dict(top=RN.const_entries(RN.TOP), top_split=RN.const_entries(RN.TOP_SPLIT), overflow=RN.const_entries(RN.OVERFLOW),
                overflow_finite32=RN.const_entries(RN.OVERFLOW_FINITE32))
    for i, e in enumerate(RN.edge_probes(dc[:2], feat)):
        sets["edge%d" % i] = e
    for name, ent in sets.items():
        assert len(ent) <= min(128, width // 2)
        net, chains = RN.range_probe(sc.n_in0, depth, width, ent, seed=3)
        names = [n for n, _ in ent]
        d = str(tmp_path_factory.mktemp("range_%s_%s" % (case, name)))
        O.write_model_dir(d, sc, O.Weights(net, filler))
        for mode in modes:
            r = context(d, mode, z, monkeypatch)
            try:
                rows = stage_rows(r, "%s %s %s" % (case, name, mode))
            finally:
                r.close()
            c, bad = check_rows(rows, feat, chains, mode, "%s %s %s" % (case, name, mode), names)
            # what the issue fixes per probe, beside the prediction
            if name == "top_split" or (name == "top" and mode != "split") or (mode == "fp32" and name != "overflow"):
                assert not bad.any() and np.isfinite(rows).all(), (case, name, mode)
            elif name in ("overflow", "overflow_finite32", "top"):
                assert bad.all() and not np.isfinite(rows).any(), (case, name, mode)
            else:      # the edge crosses the frame
                assert 0.2 * N_RAYS < bad.sum() < 0.9 * N_RAYS, (case, name, mode, int(bad.sum()))
            # one frame of a fresh context: the counter is the number of rays beyond the range (fp32 never counts)
            r = context(d, mode, z, monkeypatch)
            try:
                st = r.render_numpy()[2]
            finally:
                r.close()
            want = 0 if mode == "fp32" else int(bad.sum())
            log_figures(case, mode, name, dict(c, sampling_overflow=int(st.sampling_overflow), expected_overflow=want))
            assert st.sampling_overflow == want, "%s %s %s: sampling_overflow %d, rays beyond the range %d" % (case, name, mode, st.sampling_overflow, want)


# ---- the two-block kernel writes no rows ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["fixed_10_4", "fixed_2_2"])
def test_two_block_kernel_on_range_probes(case, scenes, base_case, filler, tmp_path_factory, monkeypatch):
    """fused frames of sample_mlp16x2_kernel ($ADANERF_DEBUG_GUARD = 4) have the bytes -- counts, offsets, keys, kept values, pixels -- of the
    8-wave kernel's (= 2), and both are the rule on the 8-wave kernel's stage rows, which test_range_probes / test_range_edges hold to the
    prediction.  Thresholds of 2^-30 and 2^-12 put the subnormal-range entries among the kept values."""
    depth, width, pe0, modes = CASES[case]
    z = base_case[0]
    sc, feat = scenes(case)
    dc, pc = T.identity_columns(sc)
    sets = dict(table=RN.table_entries(), rays=RN.ray_entries(dc, pc, feat), top_split=RN.const_entries(RN.TOP_SPLIT), edge0=RN.edge_probes(dc[:1], feat)[0])
    walk = [(16, 2.0 ** -30), (8, 2.0 ** -12), (4, 0.5)]
    for name, ent in sets.items():
        net, chains = RN.range_probe(sc.n_in0, depth, width, ent, seed=5)
        d = str(tmp_path_factory.mktemp("range_two_block_%s_%s" % (case, name)))
        O.write_model_dir(d, sc, O.Weights(net, filler))
        r = context(d, "fp16", z, monkeypatch)
        try:
            rows = stage_rows(r, "%s %s stage rows" % (case, name))
        finally:
            r.close()
        check_rows(rows, feat, chains, "fp16", "%s %s fp16" % (case, name), [n for n, _ in ent])
        frames = {}
        for dbg in ("2", "4"):
            monkeypatch.setenv("ADANERF_DEBUG_GUARD", dbg)
            with Live(d, z, W, H, 8, 0.125, sampling="fp16") as c:
                for n, thr in walk:
                    c.r.set_selection(n, thr)
                    frames[dbg, n, thr] = c.frame()[0]
        for (dbg, n, thr), f in frames.items():
            tag = "%s %s (%d, %g)" % (case, name, n, thr)
            same(f, rule(rows, n, thr), tag + " debug guard %s against the rule on the stage rows" % dbg)
            same(f, frames["2", n, thr], tag + ": the two-block kernel against the 8-wave kernel", keys=("counts", "offsets", "total", "key", "w", "rgba", "rgb"))
        record("sampling_ranges_two_block", case=case, probe=name, kernel="sample_mlp16x2_kernel", frames=len(frames), kept=[int(frames["4", n, t]["total"][0]) for n, t in walk])


# ---- a weight outside the fp16 range ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["fixed_10_4", "gen_w128_d5"])
def test_weight_outside_the_fp16_range(case, scenes, base_case, filler, tmp_path_factory, monkeypatch):
    """pack.cpp packs |w| >= 65520 as hi = inf, lo' = -inf, under which relu(-inf + bias) is a finite, wrong 0: adanerf_create refuses the
    network for every 16-bit sampling mode and runs it in ADANERF_SAMPLING_FP32, exactly"""
    depth, width, pe0, modes = CASES[case]
    z = base_case[0]
    sc, feat = scenes(case)
    for gname, g in RN.GAIN_OVER:
        ent = [(gname + " x f[0]", ("ray", 0, g))] + RN.const_entries(RN.AROUND_ONE)
        net, chains = RN.range_probe(sc.n_in0, depth, width, ent, seed=7)
        d = str(tmp_path_factory.mktemp("range_gain_%s_%s" % (case, gname)))
        O.write_model_dir(d, sc, O.Weights(net, filler))
        for mode in ("split", "fp16", "guarded"):
            with pytest.raises(adanerf_amd.AdaNeRFError, match="outside the fp16 range"):
                context(d, mode, z, monkeypatch)
        r = context(d, "fp32", z, monkeypatch)
        try:
            rows = stage_rows(r, "%s gain %s fp32" % (case, gname))
            st = r.render_numpy()[2]
        finally:
            r.close()
        c, bad = check_rows(rows, feat, chains, "fp32", "%s gain %s fp32" % (case, gname), [n for n, _ in ent])
        assert not bad.any() and st.sampling_overflow == 0
        log_figures(case, "fp32", "gain " + gname, c)
