"""The kernels around the two networks -- compositing, the inverse-CDF sampler, the fine sampler -- against the fp64 restatements of
tests/stage_reference.py, at the sizes where their dispatch branches and loop structures change:

 a. accuracy on a base set of distinct rays (stage_reference.check_composite / check_pdf / check_fine: no excluded ray, no outlier
    budget), inputs with saturating values, rows of identical samples, empty rays, multipliers in [-0.5, 1.8], and a few rays carrying
    NaN / +-inf -- those must come out non-finite in the components the fp64 reference has non-finite (compositing) or stay inside their
    own slots (samplers), and never disturb a neighbour;
 b. position invariance, no tolerance: every occurrence of a base ray in a long permuted list (threads, waves, workgroups, grid laps,
    the staged and the direct path of composite_kernel) is bit-identical to its base-set result;
 c. RGBA8 bytes equal stage_reference.rgba8_of of the fp32 colours the same launch wrote, exactly;
 d. every launch writes into exact-size outputs between two 4 KiB canary regions;
 e. the depth and accumulation maps (adanerf_composite_aux / adanerf_composite_classic_aux) of every compositing launch above: against fp64
    in the colour's units (stage_reference.check_aux, bound C_AUX: twice the fp32 emulation's worst case), signed, empty rays exactly 0;
    requested alone or together they have the same bits, a map that is not requested is not touched, and the colours beside them are the
    bits of the launch without maps; position invariance as in b.  The keys' bins ascend and differ from index & 127; the depth table
    comes from the host library.  adanerf_disp_map: bit for bit its fp32 restatement on a list of edge pairs.

Bounds: stage_reference.C (compositing, measured on an MI355X: profiles/stage_kernels_measured.log), twice the fp32 numpy oracle's
residual on the same rows (samplers).  Models are written from the golden scenes; the networks do not matter here.

Kernels and the cases that reach them:
  launch_composite
    composite_kernel<256>            test_composite[N-mult] N = 1, 8, 9          mult none / alpha / weights (mult_mode 0 / 1 / 2)
    composite_kernel<128>            N = 10, 19
    composite_kernel<64>             N = 20, 32
        each: 1, RB - 1, RB, RB + 1, 5 RB + 37 and zero rays; the compactor's layout (staged), a gapped and a reversed layout (direct),
        workgroups that span exactly cap and cap + 1 samples
    composite_wave_kernel            N = 33, 64, 65, 127, 128, threshold > 0, counts ragged in 0..N, and all counts = N;
                                     test_composite_dense_mode (threshold 0, every count 128; null key, key arange & 127, mirrored key)
        every launch: without maps (the staged / direct loops), with depth, with acc, with both (composite_kernel's map loop)
  launch_composite_classic
    composite_classic_kernel         test_composite_classic[n] n = 1, 2, 31, 32
    composite_classic_wave_kernel    n = 33, 63, 64, 65, 128, 129, 192, 1024 (1 to 16 laps, whole and ragged last laps)
  adanerf_disp_map
    disp_map_kernel                  test_disp_map[n] n = 1, 255, 256, 257, 1000
  launch_sample_pdf
    pdf_sample_kernel                test_pdf_sampler[transform-depth] n = 1, 2, 8, 63, 64, 65, 200; three laps of its grid
  launch_sample_fine / launch_sample_uniform
    fine_sample_kernel               test_fine_sampler[nc-nf] (3, 1), (3, 8), (16, 24), (64, 128), (128, 1), (128, 128); 1, 63, 64, 65, 3001 rays
    uniform_sample_kernel            the same test: ragged windows into guarded outputs"""
import dataclasses

import numpy as np
import pytest

import adanerf_oracle as O
import stage_reference as S
from conftest import load_case, record

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

PAD = 4096
MULTS = {"none": dict(accumulation_mult="alpha", losses0="MSE"),
         "alpha": dict(accumulation_mult="alpha", losses0="NeRFWeightMultiplicationLoss"),
         "weights": dict(accumulation_mult="weights", losses0="NeRFWeightMultiplicationLoss")}
COMPOSITE_N = [1, 8, 9, 10, 19, 20, 32, 33, 64, 65, 127, 128]
CLASSIC_N = [1, 2, 31, 32, 33, 63, 64, 65, 128, 129, 192, 1024]
PDF_N = [1, 2, 8, 63, 64, 65, 200]
PDF_MODELS = [("BCEWithLogitsLoss", "log"), ("BCEWithLogitsLoss", "linear"), ("CrossEntropyLoss", "log"), ("CrossEntropyLoss", "linear"),
              ("MSE", "log"), ("MSE", "linear")]
FINE_PAIRS = [(3, 1), (3, 8), (16, 24), (64, 128), (128, 1), (128, 128)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


def model_dir(tmp_path_factory, tag, sc, wts):
    d = str(tmp_path_factory.mktemp(tag))
    O.write_model_dir(d, sc, wts)
    return d


@pytest.fixture(scope="module")
def mult_dirs(tmp_path_factory):
    z, meta, sc = load_case("synthetic_fixed8")
    return {m: model_dir(tmp_path_factory, "mult_" + m, dataclasses.replace(sc, **kw), O.synthetic_weights(1)) for m, kw in MULTS.items()}


class Guarded:
    """A device output of `nbytes` between two 4 KiB canary regions; body and canaries start as 0xA5 bytes (the sentinel)."""

    def __init__(self, r, nbytes):
        self.r, self.n = r, int(nbytes)
        self.buf = r.empty((PAD + self.n + PAD,), np.uint8)
        self.buf.upload(np.full(PAD + self.n + PAD, 0xA5, np.uint8))
        self.ptr = self.buf.ptr + PAD

    def body(self, what, dtype=np.uint8):
        a = self.buf.numpy()
        assert (a[:PAD] == 0xA5).all(), what + ": wrote before the buffer"
        assert (a[PAD + self.n:] == 0xA5).all(), what + ": wrote past the buffer"
        out = a[PAD:PAD + self.n].copy().view(dtype)
        self.buf.free()
        return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


permuted = S.permuted
layout = S.layout


def _log(kernel, **ctx):
    return lambda summary: record("stage_kernel", kernel=kernel, **ctx, **summary)


def _log_aux(kernel, **ctx):
    return lambda summary: record("stage_kernel_aux", kernel=kernel, **ctx, **summary)


def untouched(g, what):
    assert (g.body(what) == 0xA5).all(), what + ": written although it was not requested"


def depth_table(r, model_dir):
    """The context's depth table from the host library -- nothing a kernel wrote"""
    return S.host_depth_table(r.lib, R._Options, model_dir, int(r.info.num_samples), float(r.info.threshold))


# ---- adaptive compositing ------------------------------------------------------------------------------------------------------------------

def run_composite(r, raw, sw, off, cnt, key, n, what, null_key=False):
    """One layout through adanerf_composite and through adanerf_composite_aux with depth only, acc only and both: every colour output of
    the four launches has the same bits, a map has the same bits whichever other map is requested, a map that is not requested is
    not touched -> rgb, rgba8, depth, acc"""
    bufs = [r.to_device(np.ascontiguousarray(a)) for a in (raw, sw, off, cnt)]
    d_key = None if null_key else r.to_device(np.ascontiguousarray(key))
    rgb, rgba = Guarded(r, n * 12), Guarded(r, n * 4)
    r.composite(*bufs, n, rgb.ptr, rgba.ptr)
    r.sync()
    K, K8 = rgb.body(what + " rgb", np.float32).reshape(n, 3), rgba.body(what + " rgba8").reshape(n, 4)
    maps = {}
    for want in ("depth", "acc", "both"):
        rgb, rgba, dm, am = Guarded(r, n * 12), Guarded(r, n * 4), Guarded(r, n * 4), Guarded(r, n * 4)
        r.composite_aux(*bufs, d_key, n, rgb.ptr, rgba.ptr, dm.ptr if want != "acc" else None, am.ptr if want != "depth" else None)
        r.sync()
        w = "%s with %s" % (what, want)
        assert same_bits(rgb.body(w + " rgb", np.float32).reshape(n, 3), K) and same_bits(rgba.body(w + " rgba8").reshape(n, 4), K8), \
            w + ": the colours differ from those of adanerf_composite"
        for name, g in (("depth", dm), ("acc", am)):
            if want in (name, "both"):
                maps.setdefault(name, []).append(g.body(w + " " + name, np.float32))
            else:
                untouched(g, w + " " + name)
    for name, (alone, both) in maps.items():
        assert same_bits(alone, both), "%s: %s alone differs from %s beside the other map" % (what, name, name)
    for b in bufs + ([] if null_key else [d_key]):
        b.free()
    return K, K8, maps["depth"][1], maps["acc"][1]


def composite_checks(r, c, N, mult, kind, tag, ztab, null_key=False):
    B = c["cnt"].shape[0]
    K, K8, D, A = run_composite(r, c["raw"], c["sw"], c["off"], c["cnt"], c["key"], B, tag, null_key)
    bins = (np.arange(c["raw"].shape[0]) if null_key else c["key"]) & 127
    ref, ref_d, ref_a, scale = S.composite64(c["raw"], c["sw"], c["off"], c["cnt"], mult, z=ztab[bins])
    name = "composite_wave_kernel" if N > 32 else "composite_kernel<%d>" % (256 if N <= 9 else 128 if N <= 19 else 64)
    S.check_composite(K, ref, scale, c["cnt"], kind, log=_log(kind, instance=name, N=N, mult=mult, case=tag))
    S.check_aux(D, A, ref_d, ref_a, scale, S.ray_zmax(ztab[bins], c["off"], c["cnt"]), c["cnt"], kind,
                log=_log_aux(kind, instance=name, N=N, mult=mult, case=tag))
    assert np.array_equal(K8, S.rgba8_of(K)), tag + ": RGBA8 is not the contract's function of the fp32 colour"
    empty = c["cnt"] == 0
    assert (~empty).any() and (K[empty] == 0).all()
    assert (D[empty].view(np.uint32) == 0).all() and (A[empty].view(np.uint32) == 0).all(), tag + ": an empty ray's maps are not +0.0"
    return K, K8, D, A


@pytest.mark.parametrize("mult", list(MULTS))
@pytest.mark.parametrize("N", COMPOSITE_N)
def test_composite(N, mult, mult_dirs):
    kind = "thread" if N <= 32 else "wave"
    RB = 256 if N <= 9 else 128 if N <= 19 else 64
    c = S.composite_inputs(1000 + N, N)
    B = c["cnt"].shape[0]
    tag = "N%d_%s" % (N, mult)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(mult_dirs[mult], 8, 8), precision="fp32", num_samples=N, threshold=0.2) as r:
        assert r.info.num_samples == N and not r.info.dense
        ztab = depth_table(r, mult_dirs[mult])
        base = composite_checks(r, c, N, mult, kind, tag, ztab)

        def same(ids, got, what):
            for name, g, k in zip(("rgb", "rgba8", "depth", "acc"), got, base):
                assert same_bits(g, k[ids]), "%s %s: %s differs from the base set" % (tag, what, name)
        counts = [1, RB - 1, RB, RB + 1, 5 * RB + 37] if kind == "thread" else [1, 3, 4, 5, 1001]
        ids = permuted(counts[-1], B)
        for n in counts:      # the compactor's layout: the staged path of composite_kernel
            same(ids[:n], run_composite(r, *layout(c, ids[:n]), n, "%s %d rays" % (tag, n)), "%d rays" % n)
        # gaps in front of every ray, and the base arrays walked backwards: the direct path
        gap = 1 + (np.arange(ids.size) % 5)
        same(ids, run_composite(r, *layout(c, ids, gap), ids.size, tag + " gapped"), "gapped")
        same(np.arange(B)[::-1], run_composite(r, c["raw"], c["sw"], c["off"][::-1].copy(), c["cnt"][::-1].copy(), c["key"], B, tag + " reversed"), "reversed")
        # every count = N: workgroups of exactly cap = RB N samples (staged); one unused slot inside each: cap + 1 (direct)
        full = np.flatnonzero(c["finite"] & (c["cnt"] == N))
        ids = full[permuted(2 * RB + 1, full.size)]
        same(ids, run_composite(r, *layout(c, ids), ids.size, tag + " cap"), "cap")
        gap = np.zeros(ids.size, np.int64)
        gap[1::RB] = 1
        same(ids, run_composite(r, *layout(c, ids, gap), ids.size, tag + " cap + 1"), "cap + 1")
        # zero rays: nothing is written; a map without a key outside the dense mode: refused, nothing is written
        bufs = [r.to_device(a) for a in (c["raw"], c["sw"], c["off"], c["cnt"])]
        d_key = r.to_device(c["key"])
        rgb, rgba = Guarded(r, 12), Guarded(r, 4)
        r.composite(*bufs, 0, rgb.ptr, rgba.ptr)
        r.sync()
        untouched(rgb, tag + " 0 rays")
        untouched(rgba, tag + " 0 rays")
        out = [Guarded(r, 12), Guarded(r, 4), Guarded(r, 4), Guarded(r, 4)]
        r.composite_aux(*bufs, d_key, 0, *[g.ptr for g in out])
        r.sync()
        for g in out:
            untouched(g, tag + " 0 rays with maps")
        for want in ((True, False), (False, True), (True, True)):
            out = [Guarded(r, B * 12), Guarded(r, B * 4), Guarded(r, B * 4), Guarded(r, B * 4)]
            with pytest.raises(adanerf_amd.AdaNeRFError, match="error -1: adanerf_composite_aux: .*d_sample_key"):
                r.composite_aux(*bufs, None, B, out[0].ptr, out[1].ptr, out[2].ptr if want[0] else None, out[3].ptr if want[1] else None)
            r.sync()
            for g in out:
                untouched(g, tag + " no key")
        rgb, rgba = Guarded(r, B * 12), Guarded(r, B * 4)      # no map: the key is not needed
        r.composite_aux(*bufs, None, B, rgb.ptr, rgba.ptr, None, None)
        r.sync()
        assert same_bits(rgb.body(tag + " no key, no map", np.float32).reshape(B, 3), base[0]) and same_bits(rgba.body(tag).reshape(B, 4), base[1])


def test_composite_dense_mode(mult_dirs):
    """threshold 0: every ray carries all 128 bins; a null key is the key arange & 127, bit for bit"""
    c2 = S.dense_layout()
    n = c2["cnt"].shape[0]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(mult_dirs["alpha"], 8, 8), precision="fp32", num_samples=128, threshold=0.0) as r:
        assert r.info.dense and r.info.num_samples == 128
        ztab = depth_table(r, mult_dirs["alpha"])
        assert np.array_equal(c2["key"] & 127, np.arange(c2["key"].shape[0], dtype=np.uint32) & 127)
        null = composite_checks(r, c2, 128, "alpha", "wave", "dense128", ztab, null_key=True)
        keyed = run_composite(r, c2["raw"], c2["sw"], c2["off"], c2["cnt"], c2["key"], n, "dense128 keyed")
        for name, a, b in zip(("rgb", "rgba8", "depth", "acc"), null, keyed):
            assert same_bits(a, b), "dense128: %s with a null key differs from the key arange & 127" % name
        # a key that is given is used in the dense mode too: every bin mirrored
        c3 = dict(c2, key=(c2["key"] & ~np.uint32(127)) | (np.uint32(127) - (c2["key"] & np.uint32(127))))
        _, _, D, A = run_composite(r, c3["raw"], c3["sw"], c3["off"], c3["cnt"], c3["key"], n, "dense128 mirrored")
        _, ref_d, ref_a, scale = S.composite64(c3["raw"], c3["sw"], c3["off"], c3["cnt"], "alpha", z=ztab[c3["key"] & 127])
        S.check_aux(D, A, ref_d, ref_a, scale, S.ray_zmax(ztab[c3["key"] & 127], c3["off"], c3["cnt"]), c3["cnt"], "wave")
        assert same_bits(A, null[3])


# ---- classic compositing ---------------------------------------------------------------------------------------------------------------------

def run_classic(r, c, ids, n, what):
    """as run_composite: adanerf_composite_classic, and adanerf_composite_classic_aux with depth only, acc only and both"""
    R_ = len(ids)
    bufs = [r.to_device(np.ascontiguousarray(c[k][ids])) for k in ("raw", "z", "rays")]
    rgb, rgba = Guarded(r, R_ * 12), Guarded(r, R_ * 4)
    r.composite_classic(*bufs, R_, n, rgb.ptr, rgba.ptr)
    r.sync()
    K, K8 = rgb.body(what + " rgb", np.float32).reshape(R_, 3), rgba.body(what + " rgba8").reshape(R_, 4)
    maps = {}
    for want in ("depth", "acc", "both"):
        rgb, rgba, dm, am = Guarded(r, R_ * 12), Guarded(r, R_ * 4), Guarded(r, R_ * 4), Guarded(r, R_ * 4)
        r.composite_classic_aux(*bufs, R_, n, rgb.ptr, rgba.ptr, dm.ptr if want != "acc" else None, am.ptr if want != "depth" else None)
        r.sync()
        w = "%s with %s" % (what, want)
        assert same_bits(rgb.body(w + " rgb", np.float32).reshape(R_, 3), K) and same_bits(rgba.body(w + " rgba8").reshape(R_, 4), K8), \
            w + ": the colours differ from those of adanerf_composite_classic"
        for name, g in (("depth", dm), ("acc", am)):
            if want in (name, "both"):
                maps.setdefault(name, []).append(g.body(w + " " + name, np.float32))
            else:
                untouched(g, w + " " + name)
    for name, (alone, both) in maps.items():
        assert same_bits(alone, both), "%s: %s alone differs from %s beside the other map" % (what, name, name)
    for b in bufs:
        b.free()
    return K, K8, maps["depth"][1], maps["acc"][1]


@pytest.mark.parametrize("n", CLASSIC_N)
def test_composite_classic(n, mult_dirs):
    kind = "classic_thread" if n <= 32 else "classic_wave"
    c = S.classic_inputs(2000 + n, n)
    B = c["z"].shape[0]
    tag = "n%d" % n
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(mult_dirs["alpha"], 8, 8), precision="fp32") as r:
        base = run_classic(r, c, np.arange(B), n, tag)
        K, K8, D, A = base
        ref, ref_d, ref_a, scale = S.composite_classic64(c["raw"], c["z"], c["rays"][:, 4:7])
        instance = "composite_classic_kernel" if n <= 32 else "composite_classic_wave_kernel"
        S.check_composite(K, ref, scale, n, kind, log=_log(kind, instance=instance, n=n, case=tag))
        S.check_aux(D, A, ref_d, ref_a, scale, np.abs(c["z"].astype(np.float64)).max(1), n, kind, log=_log_aux(kind, instance=instance, n=n, case=tag))
        assert np.array_equal(K8, S.rgba8_of(K)), tag + ": RGBA8 is not the contract's function of the fp32 colour"
        counts = [1, 255, 256, 257, 777] if kind == "classic_thread" else [1, 3, 4, 5, 1001 if n <= 192 else 301]
        ids = permuted(counts[-1], B)
        for m in counts:
            got = run_classic(r, c, ids[:m], n, "%s %d rays" % (tag, m))
            for name, g, k in zip(("rgb", "rgba8", "depth", "acc"), got, base):
                assert same_bits(g, k[ids[:m]]), "%s %d rays: %s differs from the base set" % (tag, m, name)
        bufs = [r.to_device(c[k]) for k in ("raw", "z", "rays")]
        rgb, rgba = Guarded(r, 12), Guarded(r, 4)
        r.composite_classic(*bufs, 0, n, rgb.ptr, rgba.ptr)
        r.sync()
        untouched(rgb, tag + " 0 rays")
        untouched(rgba, tag + " 0 rays")
        out = [Guarded(r, 12), Guarded(r, 4), Guarded(r, 4), Guarded(r, 4)]
        r.composite_classic_aux(*bufs, 0, n, *[g.ptr for g in out])
        r.sync()
        for g in out:
            untouched(g, tag + " 0 rays with maps")


# ---- the disparity map -----------------------------------------------------------------------------------------------------------------------

DISP_EDGES = [(0.0, 0.0), (1.0, 0.0), (-1.0, 0.0), (0.0, -0.0), (-0.0, 1.0), (-1.0, 2.0), (3.0, -0.5), (1e-12, 1.0), (1e-10, 1.0), (1.0000001e-10, 1.0),
              (9.9999e-11, 1.0), (1e-40, 1.0), (1e-40, 1e-40), (1.0, 1e-40), (1e-45, 3e-39), (-1e-40, 1.0), (3e38, 1e-3), (np.inf, 1.0),
              (-np.inf, 1.0), (np.inf, np.inf), (1.0, np.inf), (1.0, -np.inf), (np.inf, 0.0), (np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan),
              (np.nan, 0.0), (0.0, np.nan)]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_disp_map(n, mult_dirs):
    """adanerf_disp_map: bit for bit the fp32 function 1 / maximum(1e-10, depth / acc) with torch.max's (numpy.maximum's) NaN: an empty
    ray (0 / 0) stays NaN, a negative or tiny quotient meets the floor, one block and a ragged second"""
    rng = np.random.default_rng(5000 + n)
    d = rng.uniform(0.1, 9.0, n).astype(np.float32)
    a = rng.uniform(1e-3, 1.2, n).astype(np.float32)
    e = np.array(DISP_EDGES, np.float32)
    k = min(n, len(e))
    first = 0 if n >= len(e) else (n * 7) % len(e)        # n = 1: one edge pair; the long arrays: all, at both ends of the blocks
    d[:k], a[:k] = e[first:first + k, 0], e[first:first + k, 1]
    if n > 2 * len(e):
        d[-len(e):], a[-len(e):] = e[::-1, 0], e[::-1, 1]
    with np.errstate(all="ignore"):
        exp = (np.float32(1.0) / np.maximum(np.float32(1e-10), (d / a).astype(np.float32))).astype(np.float32)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(mult_dirs["alpha"], 8, 8), precision="fp32") as r:
        bufs = [r.to_device(d), r.to_device(a)]
        out = Guarded(r, n * 4)
        r.disp_map(*bufs, n, out.ptr)
        r.sync()
        got = out.body("disp_map %d" % n, np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(exp)), "NaN in other places: pairs %s" % np.flatnonzero(np.isnan(got) != np.isnan(exp))[:8].tolist()
        ok = np.isnan(exp) | (got.view(np.uint32) == exp.view(np.uint32))
        assert ok.all(), "pairs %s: %s / %s -> %s, not %s" % (np.flatnonzero(~ok)[:8].tolist(), d[~ok][:8], a[~ok][:8], got[~ok][:8], exp[~ok][:8])
        if n >= len(e):
            assert np.isnan(got[0]) and got[1] == 0.0 and got[2] == got[5] == np.float32(1.0) / np.float32(1e-10)      # 0/0, x/0, -x/0, negative
        out = Guarded(r, 4)
        r.disp_map(*bufs, 0, out.ptr)
        r.sync()
        untouched(out, "disp_map 0")
        out = Guarded(r, n * 4)
        for args in ((None, bufs[1], n, out.ptr), (bufs[0], None, n, out.ptr), (bufs[0], bufs[1], n, None), (bufs[0], bufs[1], -1, out.ptr)):
            with pytest.raises(adanerf_amd.AdaNeRFError, match="error -1"):
                r.disp_map(*args)
        r.sync()
        untouched(out, "disp_map refused")


# ---- the inverse-CDF sampler -------------------------------------------------------------------------------------------------------------------

def run_pdf(r, d_orc, R, n, what):
    off, cnt, tot = Guarded(r, R * 4), Guarded(r, R * 4), Guarded(r, 4)
    key, w, z = Guarded(r, R * n * 4), Guarded(r, R * n * 4), Guarded(r, R * n * 4)
    r.sample_pdf(d_orc, R, n, off.ptr, cnt.ptr, key.ptr, w.ptr, z.ptr, tot.ptr)
    r.sync()
    return dict(off=off.body(what + " offsets", np.int32), cnt=cnt.body(what + " counts", np.int32), total=int(tot.body(what + " total", np.int32)[0]),
                key=key.body(what + " keys", np.uint32), w=w.body(what + " weights", np.float32), z=z.body(what + " depths", np.float32))


@pytest.mark.parametrize("losses0,dt", PDF_MODELS)
def test_pdf_sampler(losses0, dt, tmp_path_factory):
    z_, meta, sc = load_case("synthetic_fixed8")
    sc = dataclasses.replace(sc, sampler="FromClassifiedDepth", losses0=losses0, depth_transform=dt)
    d = model_dir(tmp_path_factory, "pdf", sc, O.synthetic_weights(1))
    orc, fin = S.pdf_rows(3000, losses0)
    B = orc.shape[0]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 8, 8), precision="fp32") as r:
        L = 3 * int(r.info.compute_units) * 32 + 97          # three laps of the grid: compute_units * 8 workgroups of 4 rays
        ids = permuted(L, B)
        d_base, d_long = r.to_device(orc), r.to_device(np.ascontiguousarray(orc[ids]))
        for n in PDF_N:
            tag = "%s_%s_n%d" % (losses0, dt, n)
            res, _ = S.pdf_residual(O.to_world_depth(O.sample_pdf(orc[fin], n, losses0), sc), orc[fin], n, losses0, sc.depth_range, dt == "log")
            bound = S.sampler_bound(res)
            g = run_pdf(r, d_base, B, n, tag)
            S.check_pdf(g["z"], g["key"], g["w"], g["off"], g["cnt"], g["total"], orc, n, losses0, sc.depth_range, dt == "log", bound,
                        finite_rows=fin, log=_log("pdf_sample_kernel", case=tag, oracle_residual=bound / 2))
            h = run_pdf(r, d_long, L, n, tag + " long")
            assert h["total"] == L * n and (h["cnt"] == n).all() and np.array_equal(h["off"], np.arange(L, dtype=np.int32) * n)
            assert (h["w"].view(np.uint32) == 0).all()
            assert np.array_equal(h["key"].reshape(L, n) >> 7, np.repeat(np.arange(L, dtype=np.uint32)[:, None], n, 1))
            assert same_bits(h["z"].reshape(L, n), g["z"].reshape(B, n)[ids]), tag + ": depths differ from the base set"
            assert np.array_equal(h["key"].reshape(L, n) & 127, (g["key"].reshape(B, n) & 127)[ids]), tag + ": bins differ from the base set"
        g = Guarded(r, 4)
        r.sample_pdf(d_base, 0, 8, g.ptr, g.ptr, g.ptr, g.ptr, g.ptr, g.ptr)
        r.sync()
        assert (g.body("pdf 0 rays") == 0xA5).all()


# ---- the fine sampler --------------------------------------------------------------------------------------------------------------------------

def run_fine(r, raw, rays, n, tot_n, what):
    bufs = [r.to_device(np.ascontiguousarray(raw)), r.to_device(np.ascontiguousarray(rays))]
    off, cnt, tot = Guarded(r, n * 4), Guarded(r, n * 4), Guarded(r, 4)
    key, z = Guarded(r, n * tot_n * 4), Guarded(r, n * tot_n * 4)
    r.sample_from_coarse(*bufs, n, off.ptr, cnt.ptr, key.ptr, z.ptr, tot.ptr)
    r.sync()
    for b in bufs:
        b.free()
    assert int(tot.body(what + " total", np.int32)[0]) == n * tot_n
    assert (cnt.body(what + " counts", np.int32) == tot_n).all() and np.array_equal(off.body(what + " offsets", np.int32), np.arange(n, dtype=np.int32) * tot_n)
    assert np.array_equal(key.body(what + " keys", np.uint32).reshape(n, tot_n), np.repeat(np.arange(n, dtype=np.uint32)[:, None] << 7, tot_n, 1))
    return z.body(what + " depths", np.float32).reshape(n, tot_n)


def coarse_table32(sc):
    """The context's coarse depth table, computed independently of any kernel output: the host's fp32 arithmetic (model_setup.cpp:
    torch.linspace's two-sided form + 0.5 / Nc, near (1 - t) + far t, the linear depth transform), which the library compiles without
    contraction, restated operation by operation"""
    F = np.float32
    nc = sc.num_samples_coarse
    inc = F(1.0) / F(nc)
    k = np.arange(nc)
    lin = np.where(k < (nc + 1) // 2, inc * k.astype(F), F(1.0) - inc * (nc - k).astype(F)).astype(F)
    t = (lin + F(0.5 / nc)).astype(F)
    zw = (F(sc.z_near) * (F(1.0) - t) + F(sc.z_far) * t).astype(F)
    d0, d1 = F(sc.depth_range[0]), F(sc.depth_range[1])
    zc = (zw * (d1 - d0) + d0).astype(F)
    np.testing.assert_allclose(zc, O.coarse_depths(sc), rtol=1e-6, atol=0)
    return zc


@pytest.mark.parametrize("nc,nf", FINE_PAIRS)
def test_fine_sampler(nc, nf, tmp_path_factory):
    z_, meta, sc = load_case("classroom_coarse_fine_16_24")
    sc = dataclasses.replace(sc, num_samples_coarse=nc, num_samples=nf, depth_transform="linear")
    d = model_dir(tmp_path_factory, "fine", sc, O.synthetic_coarse_fine_weights(41, pos_enc=sc.pos_enc))
    c = S.fine_inputs(4000 + nc, nc)
    raw, rays, fin = c["raw"], c["rays"], c["finite"]
    B = raw.shape[0]
    tag = "nc%d_nf%d" % (nc, nf)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 8), precision="fp32") as r:
        assert r.info.num_samples == nc + nf and r.info.num_samples_coarse == nc
        r.set_camera(z_["pose"], z_["rot"])
        Z = run_fine(r, raw, rays, B, nc + nf, tag)
        zc = coarse_table32(sc)
        dirs = rays[:, 4:7]
        # a ray carrying NaN / +-inf is data: where the fp64 CDF is not finite (a NaN density in front of or inside the pdf's
        # intervals) the nf new depths come out NaN and the nc coarse depths bit for bit; every other such ray is checked like the rest
        nan_ray = ~np.isfinite(S.fine_cdf64(raw, zc, dirs)[0]).all(1)
        assert nan_ray.any() and not nan_ray[fin].any() and (~fin & ~nan_ray).any()
        for row in Z[nan_ray]:
            assert int(np.isnan(row).sum()) == nf and same_bits(row[~np.isnan(row)], zc), tag + ": a ray with a NaN density"
        fin = ~nan_ray
        zcr = np.repeat(zc[None], int(fin.sum()), 0)
        mid = (np.float32(0.5) * (zcr[:, 1:] + zcr[:, :-1])).astype(np.float32)
        orows = np.sort(np.concatenate([zcr, O.sample_pdf_bins(mid, O.classic_weights(raw[fin], zcr, dirs[fin])[:, 1:-1], nf)], -1), -1)
        bound = S.sampler_bound(S.fine_residual(S.split_fine_rows(orows.astype(np.float32), zc, nf), raw[fin], zc, dirs[fin], nf))
        S.check_fine(Z[fin], raw[fin], zc, dirs[fin], nf, bound, log=_log("fine_sample_kernel", case=tag, oracle_residual=bound / 2))
        ids = permuted(3001, B)
        for n in (1, 63, 64, 65, 3001):
            got = run_fine(r, raw[ids[:n]], rays[ids[:n]], n, nc + nf, "%s %d rays" % (tag, n))
            assert same_bits(got, Z[ids[:n]]), "%s %d rays: differs from the base set" % (tag, n)
        # the uniform coarse sampler of the same mode, ragged windows of this context's 128 rays
        for first, n in ((0, 1), (5, 63), (64, 64), (1, 127), (0, 128)):
            rr, off, cnt, tot, key = Guarded(r, n * 32), Guarded(r, n * 4), Guarded(r, n * 4), Guarded(r, 4), Guarded(r, n * nc * 4)
            r.sample_uniform(first, n, rr.ptr, off.ptr, cnt.ptr, key.ptr, tot.ptr)
            r.sync()
            what = "%s uniform (%d, %d)" % (tag, first, n)
            assert int(tot.body(what, np.int32)[0]) == n * nc and (cnt.body(what, np.int32) == nc).all()
            assert np.array_equal(off.body(what, np.int32), np.arange(n, dtype=np.int32) * nc)
            assert np.array_equal(key.body(what, np.uint32).reshape(n, nc), (np.arange(n, dtype=np.uint32)[:, None] << 7) | np.arange(nc, dtype=np.uint32)[None, :])
            assert np.isfinite(rr.body(what, np.float32)).all()
