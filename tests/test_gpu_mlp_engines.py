"""Every MLP engine instantiation launch_shade_mlp / launch_sample_mlp can reach, against an fp64 evaluation of the same operation on the
kernel's own inputs under the engine's rounding model (tests/mlp_reference.py), at ragged and multi-lap sizes:

 a. accuracy on a base set of distinct samples (rays): mlp_reference.check_engine;
 b. position invariance: every occurrence of a base sample in a long permuted list (blocks, waves, laps, tails) is bit-identical to its
    base-set output; for sampling, ragged (first_ray, n_rays) windows equal the whole-frame run;
 c. total / tail semantics of the shading kernels (d_total below, above, at zero; max_samples zero), with 4 KiB canaries on both sides of
    every output;
 d. the fp16-range contract of the split and plain-fp16 sampling engines (adanerf_stats.sampling_overflow).

Bounds: mlp_reference.BOUNDS, measured on an MI355X (profiles/mlp_engines_measured.log).  Networks are synthetic (O.synthetic_weights);
scenes and cameras are those of the golden case synthetic_fixed8, which test_oracle_golden.py pins to the reference.

Instantiations and the cases that reach them:
  launch_shade_mlp
    shade_mlp16x2_kernel <Bf16|Fp16, 10, 4>                            test_shading_engines[fixed_8x256] bf16, fp16; test_explicit_depths_inside_bins bf16
    shade_mlp32_kernel<10, 4>                                          test_shading_engines[fixed_8x256] fp32; test_explicit_depths_inside_bins fp32
    shade_mlp16_gen_staged_kernel <Bf16|Fp16, 10, 4, W> W = 64         [w40_d2_noskip], [w64_d3_skip1]
                                                        W = 128        [w96_d5_skips1_3], [w128_d6_skip2]; coarse net (test_coarse_net_...)
                                                        W = 256        [w160_d8_skips2_5], [w256_d6_skip2]
                                                        W = 512        [w257_d3_skip1], [w512_d8_skip4]
    shade_mlp16_gen_staged_kernel <Bf16|Fp16, 16, 16, W> W = 128       [w128_d4_skip0_catchall]   (its own block count)
                                                         W = 512       [w512_d2_catchall]
    shade_mlp32_gen_kernel <10, 4 | 16, 16, W = 64 / 128 / 256>        the same cases in fp32
    shade_mlp32_gen_wide_kernel <10, 4 | 16, 16>                       [w257_d3_skip1], [w512_d8_skip4], [w512_d2_catchall] in fp32
    the 16-band catch-all at widths 64 / 256 is the same template as 128 / 512 at another width; not run separately.
  launch_sample_mlp (stage calls: no fused selection; the fused forms on tie, fallback, at-threshold and non-finite rows, bit for bit:
                     test_gpu_fused_selection_edges.py; on frames of trained and random networks: test_gpu_parity.py)
    sample_mlp16x3_kernel <10, 4 | 2, 2>                               test_sampling_engines[fixed_split], [fixed_split_2_2]
    sample_mlp16_kernel<10, 4>                                         [fixed_fp16] (three laps of its persistent grid)
    sample_mlp_kernel<10, 4> (fp32 MFMA)                               [fixed_fp32]
    sample_mlp16x3_gen_kernel <10, 4 | 2, 2 | 16, 16, W = 64/128/256>  [gen_split_w*_*] (nine cases; sampling="fp16" runs it too)
    sample_mlp_gen_kernel (fp32, raySampleInput)                       [gen_fp32_w128], [gen_fp32_rsi8_w128]
    sample_mlp_gen_wide_kernel <10, 4 | 16, 16>                        [wide_fp32_w320], [wide_fp32_w512_catchall]
    the fp16-range contract: test_sampling_fp16_range_contract[fixed_split | fixed_fp16 | gen_split_w128]
    the operand rounding of every sampling kernel at the edges of its range, bit for bit (fp16 subnormals, hi = 0, ties, the last values
    below 65520 and the rays within 1 % of that edge, which the contract test above leaves out): test_gpu_sampling_ranges.py"""
import dataclasses
import math

import numpy as np
import pytest

import adanerf_oracle as O
import mlp_reference as M
from conftest import load_case, record

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

PAD = 4096
BASE = 2999            # distinct samples of the base set: prime, so prime to every block size (16, 32, 64, 128, 256)
LENGTHS = [1, 31, 32, 33, 63, 64, 65, 127, 129, 255, 257, 4097]
PREC = {"bf16": R.PREC_BF16, "fp16": R.PREC_FP16, "fp32": R.PREC_FP32}


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def base_case():
    return load_case("synthetic_fixed8")


@pytest.fixture(scope="module")
def compute_units(base_case, tmp_path_factory):
    z, meta, sc = base_case
    d = str(tmp_path_factory.mktemp("cu"))
    O.write_model_dir(d, sc, O.synthetic_weights(1))
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 8, 8), precision="fp32") as r:
        return int(r.info.compute_units)


def long_length(cu):
    """At least three laps of every persistent grid: no engine keeps more than 2 workgroups x 256 samples (rays) resident per CU --
    launch_shade_mlp: fixed 16-bit kernels min(tiles, CUs) x 256 samples (4 waves x two 32-sample blocks); staged
    16-bit kernels occupancy x 128 gen_blocks; fp32 kernels occupancy x 128 (64 in the wide form); launch_sample_mlp: the plain-fp16
    kernel occupancy x 256 rays, the split kernel occupancy x 128 rays."""
    return 3 * cu * 512 + 97


class Guarded:
    """A device output of `nbytes` between two 4 KiB canary regions; body and canaries start as 0xA5 bytes (the sentinel)."""

    def __init__(self, r, nbytes):
        self.r, self.n = r, int(nbytes)
        self.buf = r.empty((PAD + self.n + PAD,), np.uint8)
        self.buf.upload(np.full(PAD + self.n + PAD, 0xA5, np.uint8))
        self.ptr = self.buf.ptr + PAD

    def reset(self):
        self.buf.upload(np.full(PAD + self.n + PAD, 0xA5, np.uint8))

    def body(self, what):
        a = self.buf.numpy()
        assert (a[:PAD] == 0xA5).all(), what + ": wrote before the buffer"
        assert (a[PAD + self.n:] == 0xA5).all(), what + ": wrote past the buffer"
        return a[PAD:PAD + self.n]

    def free(self):
        self.buf.free()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _log(tag, **ctx):
    return lambda summary: record(tag, **ctx, **summary)


# ---- shading -------------------------------------------------------------------------------------------------------------------------

# id: (depth, width, skips, positional encoding of the shading net).  Widths run padded to 64 / 128 / 256 / 512 (pack.cpp pad_width); the
# 8 x 256 / skip 4 / 10-4 net is the fixed kernels' topology, every other one runs the run-time-shaped kernels (16-bit staged, fp32 32-row,
# fp32 wide 16-row above 256).  (6, 3) is packed into the 16-band catch-all layout.
SHADE_CASES = {
    "fixed_8x256": (8, 256, [4], (10, 4)),
    "w40_d2_noskip": (2, 40, [], (10, 4)),
    "w64_d3_skip1": (3, 64, [1], (10, 4)),
    "w96_d5_skips1_3": (5, 96, [1, 3], (10, 4)),
    "w128_d6_skip2": (6, 128, [2], (10, 4)),
    "w128_d4_skip0_catchall": (4, 128, [0], (6, 3)),
    "w160_d8_skips2_5": (8, 160, [2, 5], (10, 4)),
    "w256_d6_skip2": (6, 256, [2], (10, 4)),
    "w257_d3_skip1": (3, 257, [1], (10, 4)),
    "w512_d8_skip4": (8, 512, [4], (10, 4)),
    "w512_d2_catchall": (2, 512, [], (6, 3)),
}


def shading_model(base_case, tmp_path_factory, tag, depth, width, skips, pe1, seed):
    z, meta, sc = base_case
    sc = dataclasses.replace(sc, pos_enc=(sc.pos_enc[0], tuple(pe1)))
    wts = O.synthetic_weights(seed, n_in0=sc.n_in0, n_in1_pos=3 + 6 * pe1[0], n_in1_dir=3 + 6 * pe1[1], layers=(8, depth),
                              widths=(256, width), skip1=skips if skips else 99)
    d = str(tmp_path_factory.mktemp(tag))
    O.write_model_dir(d, sc, wts)
    return z, sc, wts, d


def base_keys(rng, n_rays, n_bins):
    """BASE distinct (ray, bin) keys in random order: random rays, the four image corners (256 x 256 frame), bins 0 and n_bins - 1"""
    corners = np.array([0, 255, 255 * 256, 256 * 256 - 1])
    rays = np.concatenate([np.repeat(corners, 2), rng.integers(0, n_rays, 3 * BASE)])
    bins = np.concatenate([np.tile([0, n_bins - 1], 4), rng.integers(0, n_bins, 3 * BASE)])
    bins[8:8 + 64:2] = 0
    bins[9:9 + 64:2] = n_bins - 1
    key = (rays.astype(np.uint32) << 7) | bins.astype(np.uint32)
    _, first = np.unique(key, return_index=True)
    keep = np.sort(first)[:BASE]          # first occurrences, in generation order: the corners and edge bins lead
    key = key[keep]
    assert key.size == BASE
    return key[rng.permutation(BASE)]


def run_shade(r, fn, d_key, total, max_samples, out, prec, long=False):
    """fn(key, total, max_samples, raw, precision, long) into the Guarded `out` (reset first); returns its body as [rows, 4] fp32.
    long: d_key is the permuted long list (an entry point with per-sample arrays besides the keys needs to know)."""
    out.reset()
    d_tot = r.to_device(np.array([total], np.int32))
    fn(d_key, d_tot, max_samples, out.ptr, PREC[prec], long)
    r.sync()
    b = out.body("raw %s total %d max %d" % (prec, total, max_samples))
    d_tot.free()
    return b.view(np.float32).reshape(-1, 4)


def shading_engine_checks(r, tag, fn, key, feat, net1, n_pos, cu, precs, bounds=None):
    """a, b and c of the module docstring for one shading engine, per precision"""
    ref64 = M.shading_mlp64(feat, net1, n_pos)
    L = long_length(cu)
    idx = (7919 * np.arange(L, dtype=np.int64) + 17) % BASE      # sample j of the long list is base sample (a j + c) mod BASE, a prime to BASE
    d_key = r.to_device(key)
    d_long = r.to_device(key[idx])
    out_base = Guarded(r, BASE * 16)
    out_long = Guarded(r, L * 16)
    SENT = np.full(4, 0xA5A5A5A5, np.uint32).view(np.float32)
    for prec in precs:
        engine = prec
        refq = ref64 if prec == "fp32" else M.shading_mlp64(feat, net1, n_pos, prec)
        K = run_shade(r, fn, d_key, BASE, BASE, out_base, prec).copy()
        M.check_engine(K, ref64, refq, engine, bounds=(bounds or {}).get(prec), log=_log("mlp_engine_shading", case=tag, prec=prec, n=BASE))
        # b: the permuted long list, and its prefixes of ragged lengths
        got = run_shade(r, fn, d_long, L, L, out_long, prec, True)
        bad = np.flatnonzero((got.view(np.uint32) != K[idx].view(np.uint32)).any(axis=1))
        assert bad.size == 0, "%s %s: %d of %d rows of the long list differ from the base set, first at %s" % (tag, prec, bad.size, L, bad[:8])
        for n in LENGTHS:
            out = Guarded(r, n * 16)
            got = run_shade(r, fn, d_long, n, n, out, prec, True)
            assert same_bits(got, K[idx[:n]]), (tag, prec, n)
            out.free()
        # c: d_total < max_samples -- rows >= d_total untouched
        t = 2500
        got = run_shade(r, fn, d_key, t, BASE, out_base, prec)
        assert same_bits(got[:t], K[:t]) and same_bits(got[t:], np.tile(SENT, (BASE - t, 1))), (tag, prec, "total < max")
        # d_total > max_samples: the first max_samples rows, nothing past them (the overshoot stays inside the canary: 200 rows < 4 KiB)
        m = 4097
        out = Guarded(r, m * 16)
        got = run_shade(r, fn, d_long, m + 200, m, out, prec, True)
        assert same_bits(got, K[idx[:m]]), (tag, prec, "total > max")
        out.free()
        # d_total == 0, and max_samples == 0: nothing is written
        got = run_shade(r, fn, d_key, 0, BASE, out_base, prec)
        assert same_bits(got, np.tile(SENT, (BASE, 1))), (tag, prec, "total == 0")
        out = Guarded(r, 0)
        run_shade(r, fn, d_key, BASE, 0, out, prec)
        out.free()
    for g in (out_base, out_long, d_key, d_long):
        g.free()


@pytest.mark.parametrize("tag", list(SHADE_CASES))
def test_shading_engines(tag, base_case, compute_units, tmp_path_factory):
    depth, width, skips, pe1 = SHADE_CASES[tag]
    z, sc, wts, d = shading_model(base_case, tmp_path_factory, "shade_" + tag, depth, width, skips, pe1, 300 + list(SHADE_CASES).index(tag))
    n_pos = 3 + 6 * pe1[0]
    rng = np.random.default_rng(77)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 256, 256), precision="fp32") as r:
        r.set_camera(z["pose"], z["rot"])
        rays = r.empty((256 * 256, 8), np.float32)
        r.ray_features(0, 256 * 256, None, rays)
        key = base_keys(rng, 256 * 256, 128)
        d_key = r.to_device(key)
        f = r.empty((BASE, sc.n_in1), np.float32)
        r.shade_features(rays, d_key, BASE, f)            # the device's own fp32 features of the base set
        feat = f.numpy()
        fn = lambda k, t, m, raw, prec, long: r.shade_mlp(rays, k, t, m, raw, prec)
        shading_engine_checks(r, tag, fn, key, feat, wts.net1, n_pos, compute_units, ("bf16", "fp16", "fp32"))


# The fused kernels encode with their own sin / cos (polynomials in the 16-bit and wide kernels); the reference is evaluated on
# adanerf_shade_features' rows.  Where the features come from the host instead (the coarse net, explicit depths) the fp32 agreement
# also carries the 2^(F-1) sensitivity of the encoding to the last bit of a position -- a bound of its own (measured, same log).
HOST_FEATURE_FP32 = {"fp32": dict(agree=1e-4)}      # measured 2.7e-5 (coarse net), 1.6e-6 (explicit depths)
# The plain-fp16 sampling kernel encodes with v_sin_f32 / v_cos_f32 (hardware, a few fp32 ulp): its fp16 operands differ from the rounded
# debug features far more often than the other engines' -- measured rms ratio 0.849, max ratio 1.27, offset 2.04 (same log)
PLAIN_FP16_SAMPLING = dict(rms_frac=1.2, max_mult=1.8, mean_z=4.0)


def test_coarse_net_of_a_coarse_fine_model(base_case, compute_units, tmp_path_factory):
    z, meta, sc = load_case("classroom_coarse_fine_16_24")
    sc = dataclasses.replace(sc, num_samples_coarse=16, num_samples=24)
    wts = O.synthetic_coarse_fine_weights(41, pos_enc=sc.pos_enc, layers=(5, 8), widths=(128, 256), skips=(1, 4))
    d = str(tmp_path_factory.mktemp("coarse"))
    O.write_model_dir(d, sc, wts)
    nc = sc.num_samples_coarse
    rng = np.random.default_rng(78)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 256, 256), precision="fp32") as r:
        r.set_camera(z["pose"], z["rot"])
        R_ = 256 * 256
        rays = r.empty((R_, 8), np.float32)
        off, cnt, tot = r.empty((R_,), np.int32), r.empty((R_,), np.int32), r.empty((1,), np.int32)
        keyc = r.empty((R_ * nc,), np.uint32)
        r.sample_uniform(0, R_, rays, off, cnt, keyc, tot)
        rec = rays.numpy()
        key = base_keys(rng, R_, nc)
        sray, sbin = (key >> 7).astype(np.int64), (key & 127).astype(np.int64)
        sc0 = dataclasses.replace(sc, pos_enc=(sc.pos_enc[0], sc.pos_enc[0]))
        feat = O.shading_inputs(rec[:, 0:3], rec[:, 4:7], sray, O.coarse_depths(sc)[sbin], sc0)
        fn = lambda k, t, m, raw, prec, long: r.shade_mlp_coarse(rays, k, t, m, raw, prec)
        shading_engine_checks(r, "coarse_w128_d5_skip1", fn, key, feat, wts.net0, 3 + 6 * sc.pos_enc[0][0], compute_units,
                              ("bf16", "fp16", "fp32"), bounds=HOST_FEATURE_FP32)


def test_explicit_depths_inside_bins(base_case, compute_units, tmp_path_factory):
    depth, width, skips, pe1 = SHADE_CASES["fixed_8x256"]
    z, sc, wts, d = shading_model(base_case, tmp_path_factory, "shade_z", depth, width, skips, pe1, 333)
    rng = np.random.default_rng(79)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 256, 256), precision="fp32") as r:
        r.set_camera(z["pose"], z["rot"])
        rays = r.empty((256 * 256, 8), np.float32)
        r.ray_features(0, 256 * 256, None, rays)
        rec = rays.numpy()
        key = base_keys(rng, 256 * 256, 128)
        sray, sbin = (key >> 7).astype(np.int64), (key & 127).astype(np.int64)
        # strictly inside the bin: t = (bin + u) / 128, u in [0.05, 0.95]
        t = ((sbin + rng.uniform(0.05, 0.95, BASE)) / 128.0).astype(np.float32)
        zw = O.to_world_depth(t, sc).astype(np.float32)
        feat = O.shading_inputs(rec[:, 0:3], rec[:, 4:7], sray, zw, sc)
        # the z array is indexed by sample like the keys: the long list has its own permuted copy (the permutation of shading_engine_checks)
        L = long_length(compute_units)
        idx = (7919 * np.arange(L, dtype=np.int64) + 17) % BASE
        d_zb, d_zl = r.to_device(zw), r.to_device(zw[idx])
        fn = lambda k, t, m, raw, prec, long: r.shade_mlp_z(rays, k, d_zl if long else d_zb, t, m, raw, prec)
        shading_engine_checks(r, "explicit_z_fixed_8x256", fn, key, feat, wts.net1, 63, compute_units, ("bf16", "fp32"), bounds=HOST_FEATURE_FP32)


# ---- sampling ------------------------------------------------------------------------------------------------------------------------

# id: (sampling mode, depth, width, positional encoding of the sampling net, raySampleInput, engine class)
SAMPLE_CASES = {
    "fixed_split": ("split", 8, 256, (10, 4), 0, "split"),
    "fixed_fp16": ("fp16", 8, 256, (10, 4), 0, "fp16"),
    "fixed_fp32": ("fp32", 8, 256, (10, 4), 0, "fp32"),
    "fixed_split_2_2": ("split", 8, 256, (2, 2), 0, "split"),
    "gen_split_w64_10_4": ("split", 4, 64, (10, 4), 0, "split"),
    "gen_split_w64_2_2": ("split", 3, 50, (2, 2), 0, "split"),
    "gen_split_w64_catchall": ("split", 5, 64, (6, 3), 0, "split"),
    "gen_split_w128_10_4": ("split", 6, 128, (10, 4), 0, "split"),
    "gen_split_w128_2_2": ("split", 4, 100, (2, 2), 0, "split"),
    "gen_split_w128_catchall": ("split", 3, 128, (6, 3), 0, "split"),
    "gen_split_w256_10_4": ("split", 6, 256, (10, 4), 0, "split"),
    "gen_split_w256_2_2": ("fp16", 5, 200, (2, 2), 0, "split"),          # run-time-shaped nets have no plain-fp16 engine: fp16 runs split
    "gen_split_w256_catchall": ("split", 2, 256, (6, 3), 0, "split"),
    "gen_fp32_w128": ("fp32", 6, 128, (10, 4), 0, "fp32"),
    "gen_fp32_rsi8_w128": ("split", 4, 128, (10, 4), 8, "fp32"),          # raySampleInput: the fp32 kernel in every mode
    "wide_fp32_w320": ("split", 5, 320, (10, 4), 0, "fp32"),              # above 256: the wide fp32 form in every mode
    "wide_fp32_w512_catchall": ("fp32", 3, 512, (6, 3), 0, "fp32"),
}
PAIRS = [(0, 1), (1, 31), (31, 32), (63, 33), (100, 63), (1000, 64), (4095, 65), (7, 127), (33, 129), (70000, 255), (12345, 257),
         (54321, 4097)]


def sampling_model(base_case, depth, width, pe0, rsi, seed):
    z, meta, sc = base_case
    sc = dataclasses.replace(sc, pos_enc=(tuple(pe0), sc.pos_enc[1]), ray_sample_input=rsi)
    wts = O.synthetic_weights(seed, n_in0=sc.n_in0, oracle_bias=0.1, oracle_scale=0.3, layers=(depth, 8), widths=(width, 256))
    return z, sc, wts


def write(tmp_path_factory, tag, sc, wts):
    d = str(tmp_path_factory.mktemp(tag))
    O.write_model_dir(d, sc, wts)
    return d


def frame_side(cu):
    return int(math.ceil(math.sqrt(long_length(cu))))


@pytest.mark.parametrize("tag", list(SAMPLE_CASES))
def test_sampling_engines(tag, base_case, compute_units, tmp_path_factory):
    mode, depth, width, pe0, rsi, engine = SAMPLE_CASES[tag]
    z, sc, wts = sampling_model(base_case, depth, width, pe0, rsi, 500 + list(SAMPLE_CASES).index(tag))
    d = write(tmp_path_factory, "sample_" + tag, sc, wts)
    side = frame_side(compute_units)
    N = side * side
    rng = np.random.default_rng(81)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, side, side), precision="bf16", sampling=mode) as r:
        r.set_camera(z["pose"], z["rot"])
        assert r.info.n_in0 == sc.n_in0
        # the whole frame in one launch: >= 3 laps of every persistent sampling grid (long_length)
        full = Guarded(r, N * 512)
        r.sample_mlp(0, N, full.ptr, None)
        r.sync()
        O_full = full.body("oracle %s whole frame" % tag).view(np.float32).reshape(N, 128).copy()
        full.free()
        # a: base set = 24 windows of 125 rays at random places + the four corners, features from the device
        starts = np.sort(rng.choice(N // 125 - 1, 24, replace=False)) * 125 + rng.integers(0, 125, 24)
        wins = [(int(s), 125) for s in starts] + [(0, 1), (side - 1, 1), (N - side, 1), (N - 1, 1)]
        fbuf = r.empty((125, sc.n_in0), np.float32)
        feats, rows = [], []
        for s, n in wins:
            r.ray_features(s, n, fbuf, None)
            feats.append(fbuf.numpy()[:n].copy())
            rows.append(np.arange(s, s + n))
        feat, rows = np.concatenate(feats), np.concatenate(rows)
        K = O_full[rows]
        ref64 = M.sampling_mlp64(feat, wts.net0)
        refq = ref64 if engine == "fp32" else M.sampling_mlp64(feat, wts.net0, engine)
        M.check_engine(K, ref64, refq, engine, bounds=PLAIN_FP16_SAMPLING if tag == "fixed_fp16" else None,
                       log=_log("mlp_engine_sampling", case=tag, mode=mode, n=int(rows.size)))
        # b: ragged windows equal the whole-frame run, bit for bit; one of them with the ray records too
        for first, n in PAIRS + [(N - 97, 97), (97, N - 97)]:
            out = Guarded(r, n * 512)
            rays_out = Guarded(r, n * 32) if n == 257 else None
            r.sample_mlp(first, n, out.ptr, rays_out.ptr if rays_out else None)
            r.sync()
            got = out.body("oracle %s (%d, %d)" % (tag, first, n)).view(np.float32).reshape(n, 128)
            assert same_bits(got, O_full[first:first + n]), (tag, first, n)
            if rays_out:
                rays_out.body("rays %s" % tag)
                rays_out.free()
            out.free()
        # n_rays == 0 writes nothing
        out = Guarded(r, 512)
        r.sample_mlp(5, 0, out.ptr, None)
        r.sync()
        assert (out.body("oracle %s n_rays 0" % tag) == 0xA5).all()
        out.free()


# ---- d: the fp16-range contract of the split and plain-fp16 sampling engines ------------------------------------------------------------

F16_EDGE = 65520.0      # the smallest value that rounds to inf in fp16 (RNE)

OVERFLOW_CASES = {"fixed_split": ("split", 8, 256), "fixed_fp16": ("fp16", 8, 256), "gen_split_w128": ("split", 6, 128)}


@pytest.mark.parametrize("tag", list(OVERFLOW_CASES))
def test_sampling_fp16_range_contract(tag, base_case, tmp_path_factory):
    mode, depth, width = OVERFLOW_CASES[tag]
    z, meta, sc = base_case
    w, h = 64, 48
    wts = O.synthetic_weights(600, n_in0=sc.n_in0, oracle_bias=0.1, oracle_scale=0.3, layers=(depth, 8), widths=(width, 256))
    d0 = write(tmp_path_factory, "ovf_probe_" + tag, sc, wts)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d0, w, h), precision="bf16", sampling="fp32") as r:
        r.set_camera(z["pose"], z["rot"])
        fb = r.empty((w * h, sc.n_in0), np.float32)
        r.ray_features(0, w * h, fb, None)
        feat = fb.numpy()
    # scale hidden layer 2 (weights and bias) so that about half of the rays carry a hidden activation >= F16_EDGE in fp64
    L = 2
    m1 = M.sampling_hidden_max(feat, wts.net0)
    s = F16_EDGE / np.quantile(m1, 0.5)
    net0 = dict(wts.net0)
    net0["layers.%d.weight" % L] = (net0["layers.%d.weight" % L] * s).astype(np.float32)
    net0["layers.%d.bias" % L] = (net0["layers.%d.bias" % L] * s).astype(np.float32)
    wts = O.Weights(net0, wts.net1)
    m = M.sampling_hidden_max(feat, net0)
    over = m >= F16_EDGE
    keep = np.abs(m / F16_EDGE - 1.0) > 0.01            # rays within 1 % of the edge are left out
    assert 0.1 < over[keep].mean() < 0.9, over[keep].mean()
    d = write(tmp_path_factory, "ovf_" + tag, sc, wts)
    ref64 = M.sampling_mlp64(feat, net0)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h), precision="bf16", sampling=mode) as r:
        r.set_camera(z["pose"], z["rot"])
        ob = r.empty((w * h, 128), np.float32)
        r.sample_mlp(0, w * h, ob, None)
        orc = ob.numpy()
    bad = ~np.isfinite(orc).all(axis=1)
    wrong = np.flatnonzero(keep & (bad != over))
    record("mlp_engine_overflow", case=tag, mode=mode, rays=int(w * h), expected=int(over[keep].sum()), left_out=int((~keep).sum()),
           non_finite=int(bad.sum()), wrong=[int(i) for i in wrong[:16]], n_wrong=int(wrong.size),
           missed=int((keep & over & ~bad).sum()), spurious=int((keep & ~over & bad).sum()))
    assert wrong.size == 0, "%s: %d rays disagree with the fp64 range test (missed %d, spurious %d): %s" % (
        tag, wrong.size, int((keep & over & ~bad).sum()), int((keep & ~over & bad).sum()), wrong[:16])
    # the rays the engine can finish stay exact: the finite rows within the split / fp16 bound of fp64
    ok = ~over & keep
    engine = "fp16" if mode == "fp16" else "split"
    M.check_engine(orc[ok], ref64[ok], M.sampling_mlp64(feat[ok], net0, engine), engine, bounds=PLAIN_FP16_SAMPLING if engine == "fp16" else None,
                   log=_log("mlp_engine_overflow_finite", case=tag))
    # one frame in a fresh context (the counter runs since create): the counter equals the rays the stage found non-finite
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h), precision="bf16", sampling=mode) as r:
        r.set_camera(z["pose"], z["rot"])
        _, _, st = r.render_numpy()
    record("mlp_engine_overflow_frame", case=tag, sampling_overflow=int(st.sampling_overflow), non_finite=int(bad.sum()))
    assert st.sampling_overflow == int(bad.sum()), (st.sampling_overflow, int(bad.sum()))
    # the same net in fp32: finite, within the fp32 bound of fp64, no overflow counted
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h), precision="bf16", sampling="fp32") as r:
        r.set_camera(z["pose"], z["rot"])
        ob = r.empty((w * h, 128), np.float32)
        r.sample_mlp(0, w * h, ob, None)
        orc32 = ob.numpy()
        _, _, st = r.render_numpy()
    M.check_engine(orc32, ref64, ref64, "fp32", log=_log("mlp_engine_overflow_fp32", case=tag))
    assert st.sampling_overflow == 0
