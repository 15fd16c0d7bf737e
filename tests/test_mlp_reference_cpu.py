"""CPU checks of tests/mlp_reference.py: the fp64 evaluation agrees with the oracle's fp32 networks, the bf16 / fp16 / split rounding models
agree with numpy replays of the library's own packed weights (fixed, run-time-shaped and wide layouts), and the comparator that the GPU engine
tests use accepts a correct fp32 emulation while rejecting each emulated kernel fault."""
import numpy as np
import pytest

import adanerf_oracle as O
import mlp_reference as M
from conftest import case_weights, load_case
from mfma_emulation import PackedNet, pack_weights, run_sampling_net, run_shading_net, run_shading_net_generic
from test_host_cpu import _model_dir

import adanerf_amd
from adanerf_amd import renderer as R

PREC = {"bf16": 0, "fp16": 1, "fp32": 2, "split": 3}


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


def _unit(v):
    return (v / np.sqrt(np.sum(v * v, -1, keepdims=True))).astype(np.float32)


def shading_inputs(n, fp=10, fd=4, seed=0):
    """normalised positions in [-1, 1]^3 and unit directions -> (x, d, [PE_pos(x) | PE_dir(d)])"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    d = _unit(rng.standard_normal((n, 3)).astype(np.float32))
    return x, d, np.concatenate([O.positional_encoding(x, fp), O.positional_encoding(d, fd)], 1)


def sampling_inputs(n, fp=10, fd=4, seed=1):
    """unit directions and sphere-exit-like points (|p| ~ 1..3) -> (u, p, [PE_dir(u) | PE_pos(p)])"""
    rng = np.random.default_rng(seed)
    u = _unit(rng.standard_normal((n, 3)).astype(np.float32))
    p = (u * rng.uniform(1, 3, (n, 1))).astype(np.float32)
    return u, p, np.concatenate([O.positional_encoding(u, fd), O.positional_encoding(p, fp)], 1)


@pytest.mark.parametrize("name", ["synthetic_fixed8", "syn_6x128_skip2", "syn_7x128_skips_1_4", "syn_w40_w70_skip1", "syn_w320_w512_skip4",
                                  "syn_enc_6-3_12-2"])
def test_exact_model_matches_the_fp32_oracle(name):
    z, meta, sc = load_case(name)
    wts = case_weights(meta)
    n_pos = 3 + 6 * sc.pos_enc[1][0]
    x1 = z["shade_in"]
    a, b = M.shading_mlp64(x1, wts.net1, n_pos), O.shading_mlp(x1, wts.net1, n_pos)
    assert np.abs(a - b).max() <= 2e-5 * max(1.0, np.abs(a).max()), np.abs(a - b).max()
    x0 = z["oracle_in"]
    a, b = M.sampling_mlp64(x0, wts.net0), O.sampling_mlp(x0, wts.net0)
    assert np.abs(a - b).max() <= 2e-5 * max(1.0, np.abs(a).max()), np.abs(a - b).max()


# (depth, width, skips): the fixed 8 x 256 layout, the run-time-shaped 32-row layout at a padded width, and the 16-bit layout at width 512
SHADING_LAYOUTS = [(8, 256, [4]), (5, 96, [1, 3]), (4, 320, [1])]


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("depth,width,skips", SHADING_LAYOUTS)
def test_rounding_models_match_the_packed_shading_replays(lib, tmp_path, prec, depth, width, skips):
    """The numpy replay of the packed 16-bit fragments (what the kernels read) is a correct emulation in fp32 with the kernels' k order:
    the comparator must accept it against the bf16 / fp16 model, which ties the model's rounding points to the packer."""
    wts = O.synthetic_weights(11 + depth, layers=(8, depth), widths=(256, width), skip1=skips)
    d, _, _ = _model_dir(tmp_path, weights=wts)
    w, b, lay = pack_weights(lib, d, 1, PREC[prec])
    pn = PackedNet(w, b, lay, PREC[prec])
    x, dirs, feat = shading_inputs(1500)
    if (depth, width, skips) == (8, 256, [4]):
        K = run_shading_net(pn, x, dirs)
    else:
        K = run_shading_net_generic(pn, x, dirs, depth, 128 if width <= 128 else 256 if width <= 256 else 512, skips)
    ref64 = M.shading_mlp64(feat, wts.net1, 63)
    refq = M.shading_mlp64(feat, wts.net1, 63, prec)
    M.check_engine(K, ref64, refq, prec)


def test_split_model_matches_the_packed_sampling_replay(lib, tmp_path):
    wts = O.synthetic_weights(5)
    d, _, _ = _model_dir(tmp_path, weights=wts)
    w, b, lay = pack_weights(lib, d, 0, 3)
    u, p, feat = sampling_inputs(600)
    K = run_sampling_net(PackedNet(w, b, lay, 3), u, p, 10, 4)
    ref64 = M.sampling_mlp64(feat, wts.net0)
    refq = M.sampling_mlp64(feat, wts.net0, "split")
    M.check_engine(K, ref64, refq, "split")
    # the split model is within fp32 summation noise of the replay; plain fp16 operands would be three orders of magnitude off
    assert np.abs(K - refq).max() < 1e-5
    assert np.abs(M.sampling_mlp64(feat, wts.net0, "fp16") - ref64).max() > 100 * np.abs(K - refq).max()


# ---- discrimination: the comparator accepts a correct emulation and rejects each emulated fault ----------------------------------------------

def prev_block(K, block=32):
    """the fault: the last partial block's rows are the previous block's"""
    K = K.copy()
    n = K.shape[0]
    t = n % block
    assert t and n > block
    K[n - t:] = K[n - t - block:n - block]
    return K


# Faults by engine class.  Not every fault applies everywhere, and two cannot be caught where they are left out:
#  - "rtz" (one layer's activations rounded toward zero) for fp32 and split: the fp32 engines round no operand; the split engines' lo' part
#    carries the rounding at 2^-22 relative, below fp32 summation noise -- truncating it is indistinguishable from a different k order.
#  - "plain_fp16" (one layer in plain fp16 instead of split) is a fault of the split engines only.
#  - "skip_shift" needs a skip: shading networks only.
SHADE_FAULTS = {"bf16": ["drop_bias", "skip_shift", "rtz", "prev_block", "pad"], "fp16": ["drop_bias", "skip_shift", "rtz", "prev_block", "pad"],
                "fp32": ["drop_bias", "skip_shift", "prev_block", "pad"]}
SAMPLE_FAULTS = {"split": ["drop_bias", "plain_fp16", "prev_block"], "fp16": ["drop_bias", "rtz", "prev_block"],
                 "fp32": ["drop_bias", "prev_block", "pad"]}
N = 2003      # ragged: 62 full 32-sample blocks + 19


def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


@pytest.mark.parametrize("engine", list(SHADE_FAULTS))
def test_comparator_discriminates_shading_faults(engine):
    depth, width, skips = 4, 288, [1]      # a width that runs padded to 512; layer 2 takes the skip concatenation
    wts = O.synthetic_weights(21, layers=(8, depth), widths=(256, width), skip1=skips)
    net = wts.net1
    _, _, feat = shading_inputs(N, seed=3)
    model = "exact" if engine == "fp32" else engine
    ref64 = M.shading_mlp64(feat, net, 63)
    refq = M.shading_mlp64(feat, net, 63, model)
    ok = M.shading_mlp64(feat, net, 63, model, f32=True)
    M.check_engine(ok, ref64, refq, engine)
    for fault in SHADE_FAULTS[engine]:
        if fault == "prev_block":
            K = prev_block(ok)
        elif fault == "pad":
            K = M.shading_mlp64(feat, M.pad_with_garbage(net, "pts_linears.", 2), 63, model, f32=True)
        else:
            K = M.shading_mlp64(feat, net, 63, model, fault=(fault, 1 if fault == "skip_shift" else 2), f32=True)
        _rejected(lambda: M.check_engine(K, ref64, refq, engine))


@pytest.mark.parametrize("engine", list(SAMPLE_FAULTS))
def test_comparator_discriminates_sampling_faults(engine):
    width = 288 if engine == "fp32" else 256      # split / plain fp16 packings stop at 256; the fp32 one pads 288 to 512
    wts = O.synthetic_weights(23, layers=(5, 8), widths=(width, 256))
    net = wts.net0
    _, _, feat = sampling_inputs(N, seed=4)
    model = "exact" if engine == "fp32" else engine
    ref64 = M.sampling_mlp64(feat, net)
    refq = M.sampling_mlp64(feat, net, model)
    ok = M.sampling_mlp64(feat, net, model, f32=True)
    M.check_engine(ok, ref64, refq, engine)
    for fault in SAMPLE_FAULTS[engine]:
        if fault == "prev_block":
            K = prev_block(ok)
        elif fault == "pad":
            K = M.sampling_mlp64(feat, M.pad_with_garbage(net, "layers.", 2), model, f32=True)
        else:
            K = M.sampling_mlp64(feat, net, model, fault=(fault, 2), f32=True)
        _rejected(lambda: M.check_engine(K, ref64, refq, engine))
