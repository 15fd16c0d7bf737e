"""Hidden widths 257..512 (run zero-padded to 512, pack.cpp pad_width), CPU side: the loader accepts the wide fixtures, the fp32
packing of either net (the wide 16-row form, layout.hpp act_feature_wide) and the 16-bit packings of the shading net replay in numpy
to the reference's / the oracle's outputs, the packings the kernels do not have are refused with a message, and the new kernel
instantiations keep off scratch and within the CU's LDS."""
import ctypes as C
import re

import numpy as np
import pytest

import adanerf_oracle as O
import test_oracle_golden as TOG
from conftest import case_weights, load_case
from mfma_emulation import PackedNet, _decode, pack_weights, pe_eval, run_sampling_net_generic, run_shading_net_generic
from test_host_cpu import _device_assembly, _model_dir, _opts

import adanerf_amd
from adanerf_amd import renderer as R

WIDE_CASES = ["syn_w320_w512_skip4", "syn_w256_w384_skips_1_4"]


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


def pad(w):
    return 64 if w <= 64 else 128 if w <= 128 else 256 if w <= 256 else 512


# ---- numpy replay of the wide fp32 form (k_generic_f32.hip.hpp layer_f32_wide): four lane groups g, 16-row tiles ----------------------

def pe_wide(x, F):
    """[n,3] -> [4, pe_slots(F) / 2, n]: slot q of group g = the 32-row form's slot 2 q + (g >> 1) of lane-half g & 1"""
    p = pe_eval(x, F)
    return np.stack([p[g & 1, (g >> 1)::2] for g in range(4)])


def layer_wide(net, l, act, relu):
    """act [4, QS, n] -> [4, 4 MT, n]: D[16 m + i] = sum_g sum_q A[m][q][g, i] act[g, q]; lane (i, g) keeps rows 4 g + r"""
    w_off, b_off, QS, MT = [int(v) for v in net.lay[l]]
    assert act.shape[1] == QS, (act.shape, QS)
    frag = _decode(net.w[w_off * 16:(w_off + MT * (QS // 4) * 64) * 16], 2).reshape(MT, QS // 4, 64, 4)
    bias = net.b[b_off:b_off + MT * 16].reshape(MT, 4, 4)
    n = act.shape[2]
    out = np.zeros((4, 4 * MT, n), dtype=np.float32)
    for m in range(MT):
        D = np.zeros((16, n), dtype=np.float32)
        for g in range(4):
            D += frag[m, :, 16 * g:16 * (g + 1), :].transpose(1, 0, 2).reshape(16, QS) @ act[g]
        for g in range(4):
            out[g, 4 * m:4 * m + 4] = D[4 * g:4 * g + 4] + bias[m, g][:, None]
    return np.maximum(out, 0) if relu else out


def run_sampling_net_wide(net, dir_unit, p, fp, fd):
    depth = net.lay.shape[0]
    act = layer_wide(net, 0, np.concatenate([pe_wide(dir_unit, fd), pe_wide(p, fp)], axis=1), True)
    for l in range(1, depth - 1):
        act = layer_wide(net, l, act, True)
    out = layer_wide(net, depth - 1, act, False)      # [4, 32, n]: bin 16 m + 4 g + r
    orc = np.zeros((out.shape[2], 128), dtype=np.float32)
    for g in range(4):
        for q in range(32):
            orc[:, 16 * (q >> 2) + 4 * g + (q & 3)] = out[g, q]
    return orc


def run_shading_net_wide(net, x, dpe, depth, skips, fp=10, fd=4):
    pts, dirs = pe_wide(x, fp), pe_wide(dpe, fd)
    h = layer_wide(net, 0, pts, True)
    for l in range(1, depth):
        h = layer_wide(net, l, np.concatenate([pts, h], axis=1) if (l - 1) in skips else h, True)
    f = layer_wide(net, depth, h, False)      # 33 tiles: the alpha row is tile 32, row 0 -> group 0, slot 128
    v = layer_wide(net, depth + 1, np.concatenate([f[:, :128], dirs], axis=1), True)
    rgb = layer_wide(net, depth + 2, v, False)
    return np.stack([rgb[0, 0], rgb[0, 1], rgb[0, 2], f[0, 128]], axis=1)


def _pack_rc(lib, d, net, prec):
    f = lib.adanerf_host_pack_weights
    wb, bf, nl = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
    rc = f(d.encode(), net, prec, None, C.byref(wb), None, C.byref(bf), None, C.byref(nl))
    return rc, (lib.adanerf_last_error(None) or b"").decode()


@pytest.mark.parametrize("name", WIDE_CASES)
def test_wide_networks_pack_and_reproduce_the_reference(lib, tmp_path, name):
    z, meta, sc = load_case(name)
    wts = case_weights(meta)
    d, _, _ = _model_dir(tmp_path, sc, wts, name=name)
    syn = meta["syn"]
    w0, w1 = syn["widths"]
    assert max(w0, w1) > 256
    # the loader: both fp32 packings exist for the model (today's code refuses every width above 256)
    for net in (0, 1):
        rc, msg = _pack_rc(lib, d, net, 2)
        assert rc == 0, msg
    lib.adanerf_host_parse_model.argtypes = [C.c_char_p, C.POINTER(R._Options), C.POINTER(R.Info)]
    info = R.Info()
    assert lib.adanerf_host_parse_model(d.encode(), C.byref(_opts(width=meta["w"], height=meta["h"])), C.byref(info)) == 0
    assert info.n_in0 == sc.n_in0
    fp, fd = sc.pos_enc[0]
    n = 48
    nds = z["nds"][:n]
    u = (nds / np.sqrt(np.sum(nds * nds, -1, keepdims=True))).astype(np.float32)
    # sampling net: fp32 fragments, the wide form above 256 (16-row tiles, 128 slots per group), else today's layout
    w, b, lay = pack_weights(lib, d, 0, 2)
    net0 = PackedNet(w, b, lay, 2)
    assert lay.shape[0] == syn["layers"][0]
    if pad(w0) == 512:
        assert [int(v) for v in lay[:, 3]] == [32] * (syn["layers"][0] - 1) + [8]
        assert [int(v) for v in lay[1:, 2]] == [128] * (syn["layers"][0] - 1)
        orc = run_sampling_net_wide(net0, u, z["p"][:n], fp, fd)
    else:
        orc = run_sampling_net_generic(net0, u, z["p"][:n], nds, fp, fd)
    np.testing.assert_allclose(orc, z["oracle_out"][:n], rtol=0, atol=1e-4)
    # shading net on a few of the fixture's samples against the oracle
    count = z["sel_count"].astype(np.int32)
    off, sray, sbin, sw = O.compact(count, z["sel_bins"], z["sel_weight"])
    feat = O.shading_inputs(z["p"], z["nds"], sray[:n], O.to_world_depth(O.bin_t(sbin[:n].astype(np.int64)), sc), sc)
    ref = O.shading_mlp(feat, wts.net1)
    depth, skips = O.shading_topology(wts.net1, 63)
    assert pad(w1) == 512
    w, b, lay = pack_weights(lib, d, 1, 2)
    assert lay.shape[0] == depth + 3 and [int(v) for v in lay[:, 3]] == [32] * depth + [33, 16, 1]
    out = run_shading_net_wide(PackedNet(w, b, lay, 2), feat[:, 0:3], feat[:, 63:66], depth, list(skips))
    np.testing.assert_allclose(out, ref, rtol=0, atol=2e-4)
    # 16-bit shading keeps the 32-row form at width 512 (k_generic16.hip.hpp); bf16 packs scaled -- every exponent finite (PackedNet.layer
    # asserts that no scaled ReLU layer exceeds 1)
    for prec, tol in ((0, 0.25), (1, 0.03)):
        wq, bq, layq = pack_weights(lib, d, 1, prec)
        pn = PackedNet(wq, bq, layq, prec)
        assert [int(v) for v in pn.lay[:, 3]] == [16] * depth + [17, 8, 1]
        if prec == 0:
            assert pn.scaled and all(abs(e) <= 100 for e in pn.out_exp)
        outq = run_shading_net_generic(pn, feat[:, 0:3], feat[:, 63:66], depth, 512, list(skips))
        assert np.abs(outq - ref).max() < tol and np.sqrt(np.mean((outq - ref) ** 2)) < tol / 6, prec


@pytest.mark.parametrize("name", WIDE_CASES)
def test_numpy_oracle_reproduces_the_wide_fixtures(name):
    TOG.test_world_rays_and_oracle_features(name)
    TOG.test_sampling_mlp(name)
    TOG.test_end_to_end_rgb(name)


def test_wide_sampling_nets_refuse_the_16_bit_packings(lib, tmp_path):
    z, meta, sc = load_case("syn_w320_w512_skip4")
    d, _, _ = _model_dir(tmp_path, sc, case_weights(meta), name="wide0")
    for prec in (1, 3):      # plain fp16, split pairs
        rc, msg = _pack_rc(lib, d, 0, prec)
        assert rc != 0 and "256" in msg and "fp32" in msg, (prec, msg)
    # the 8 x 256 sampling net of the other fixture keeps its split packing
    z, meta, sc = load_case("syn_w256_w384_skips_1_4")
    d, _, _ = _model_dir(tmp_path, sc, case_weights(meta), name="narrow0")
    assert _pack_rc(lib, d, 0, 3)[0] == 0


@pytest.mark.parametrize("width", [513, 1024])
def test_widths_above_512_are_refused_with_a_message(lib, tmp_path, width):
    z, meta, sc = load_case("syn_w320_w512_skip4")
    for net, widths in ((0, (width, 128)), (1, (128, width))):
        wts = O.synthetic_weights(7, n_in0=sc.n_in0, layers=(3, 3), widths=widths, skip1=1)
        d, _, _ = _model_dir(tmp_path, sc, wts, name="w%d_%d" % (width, net))
        for prec in (0, 2):
            if net == 0 and prec == 0:
                continue
            rc, msg = _pack_rc(lib, d, net, prec)
            assert rc != 0 and str(width) in msg and "512" in msg, (net, prec, msg)
        # and the context refuses it before touching a device
        o = _opts(width=64, height=48, precision=2)
        ctx = C.c_void_p()
        assert lib.adanerf_create(d.encode(), C.byref(o), C.byref(ctx)) != 0
        assert "512" in (lib.adanerf_last_error(None) or b"").decode()


def _kernels(text):
    out = {}
    for k in re.split(r"\n\s*\.globl\s+", text)[1:]:
        name = k.split("\n", 1)[0].strip()
        if ".amdhsa_kernel" in k:
            out[name] = k
    return out


def test_wide_kernels_assembly():
    """The width-512 instantiations: the wide fp32 kernels and the staged 16-bit shading kernel (one block per wave, one workgroup per CU),
    named explicitly -- no scratch, LDS within the CU's 160 KiB, and the staged kernel drains its LDS-DMA before s_endpgm."""
    text = _device_assembly()
    if text is None:
        pytest.skip("no hipcc")
    ks = _kernels(text)
    want = ["_ZN7adanerf26sample_mlp_gen_wide_kernelILi10ELi4EEEvNS_10SampleArgsENS_11GenericTopoE",
            "_ZN7adanerf26sample_mlp_gen_wide_kernelILi2ELi2EEEvNS_10SampleArgsENS_11GenericTopoE",
            "_ZN7adanerf26sample_mlp_gen_wide_kernelILi16ELi16EEEvNS_10SampleArgsENS_11GenericTopoE",
            "_ZN7adanerf27shade_mlp32_gen_wide_kernelILi10ELi4EEEvNS_9ShadeArgsENS_11GenericTopoE",
            "_ZN7adanerf27shade_mlp32_gen_wide_kernelILi16ELi16EEEvNS_9ShadeArgsENS_11GenericTopoE"]
    staged = ["_ZN7adanerf29shade_mlp16_gen_staged_kernelINS_4%sELi%dELi%dELi512ELi1ELi1EEEvNS_9ShadeArgsENS_11GenericTopoE" % (et, fp, fd)
              for et in ("Bf16", "Fp16") for fp, fd in ((10, 4), (16, 16))]
    for name in want + staged:
        assert name in ks, name
        k = ks[name]
        get = lambda key: int(re.search(r"\.amdhsa_" + key + r"\s+(\d+)", k).group(1))
        assert get("private_segment_fixed_size") == 0, name
        assert get("group_segment_fixed_size") <= 160 * 1024, name
        assert get("next_free_vgpr") <= 512, name
        assert "v_mfma_f32_16x16x4" in k if name in want else "v_mfma_f32_32x32x16" in k, name
        if name in staged:
            body = k.split(".end_amdhsa_kernel")[0]
            lines = [ln.split(";")[0].strip() for ln in body.split("\n")]
            lines = [ln for ln in lines if ln and not ln.startswith(".")]
            dma = [i for i, ln in enumerate(lines) if re.match(r"(buffer|global)_load_\w+ .*\blds\b", ln)]
            ends = [i for i, ln in enumerate(lines) if ln.startswith("s_endpgm")]
            assert dma and ends, name
            assert any(re.match(r"s_waitcnt\b.*vmcnt\(0\)", ln) for ln in lines[dma[-1] + 1:ends[-1]]), name
