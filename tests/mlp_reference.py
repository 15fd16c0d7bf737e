"""fp64 evaluation of the two networks under explicit rounding models, and the comparator every MLP engine test uses.

Networks come as the oracle's weight dicts (``O.Weights.net0`` / ``.net1``), inputs as fp32 feature rows.  Rounding models:

- ``exact``: fp64 throughout.
- ``bf16`` / ``fp16``: every operand of a matrix product is rounded to the MFMA operand type (RNE, ``mfma_emulation.quantize``): the
  weights, the encoded inputs (identity slots included), every ReLU output, the skip concatenation (which reuses the rounded
  encoding) and ``feature_linear``'s output feeding ``views_linears.0``.  Biases and accumulation stay exact.  The bf16 packer's
  per-layer powers of two (pack.cpp scale_layer) commute with every rounding on the way and are not modelled.
- ``split``: every operand is ``hi + 2^-11 lo'`` with both parts fp16 (pack.cpp F16_SPLIT, k_sampling16.hip.hpp split_pack), and a
  product keeps ``hi*hi + hi*lo' + lo'*hi`` (the ``lo'*lo'`` term, 2^-22 relative, is dropped as the kernels drop it).

Faults (``fault=(kind, layer)``) are the emulated kernel bugs the CPU suite shows the comparator rejects (tests/test_mlp_reference_cpu.py).
"""
import numpy as np

from mfma_emulation import quantize

MODELS = ("exact", "bf16", "fp16", "split")
SPLIT = 2048.0

# Bounds of check_engine, per engine class.  Every constant is measured on an MI355X (profiles/mlp_engines_measured.log, one line per engine
# and case) and kept a stated margin above the worst case there:
#  16-bit engines: rms(K - refq) <= rms_frac * rms(refq - ref64) and max|K - refq| <= max_mult * max|refq - ref64| per output column --
#                  fp32 accumulation in another order flips roundings of activations near a midpoint, so K is not refq; it is noise around it:
#                  |mean(K - refq)| sqrt(n) <= mean_z * rms(refq - ref64) (a systematic offset, e.g. a lost bias term, is not noise);
#                  |K - ref64| <= intrinsic * scale.
#  fp32 / split:   |K - ref64| <= agree * scale (the kernel's own arithmetic against fp64 on its inputs).
#  scale = max(1, max|ref64| of the column): the synthetic nets' outputs are O(1); deeper / wider ones reach a few units.
BOUNDS = {
    "bf16": dict(rms_frac=0.35, max_mult=1.2, mean_z=4.0, intrinsic=0.05),      # worst measured 0.226, 0.807, 0.33, 0.0233
    "fp16": dict(rms_frac=0.8, max_mult=2.0, mean_z=4.0, intrinsic=0.006),      # worst measured 0.605, 1.451, 1.01, 0.0034
    "split": dict(agree=3e-6),                                                  # worst measured 1.3e-6 (stated on the shipped weights: 1.9e-6)
    "fp32": dict(agree=5e-6),                                                   # worst measured 2.5e-6
}


def _round(x, model):
    if model == "bf16":
        return quantize(np.asarray(x, np.float32), 0).astype(np.float64)
    if model == "fp16":
        return quantize(np.asarray(x, np.float32), 1).astype(np.float64)
    return np.asarray(x, np.float64)


def _rtz(x, model):
    """round toward zero to the operand type (the fault: truncation where the kernels round to nearest even)"""
    x32 = np.asarray(x, np.float32)
    if model == "bf16":
        return (x32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    h = x32.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x32)
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float64)


def split_parts(x):
    """fp32 value -> (hi, lo') as float64: hi = fp16(x), lo' = fp16((x - hi) * 2^11)"""
    x32 = np.asarray(x, np.float32)
    hi = x32.astype(np.float16).astype(np.float32)
    lo = ((x32 - hi) * np.float32(SPLIT)).astype(np.float16).astype(np.float32)
    return hi.astype(np.float64), lo.astype(np.float64)


def linear(x, w, b, model, fault_here=None, f32=False):
    """x [n, k] @ w.T + b in float64 with the operands rounded as `model` rounds them (x: fp32-representable activations).
    f32: the same operands multiplied and summed in fp32 in the reverse k order (an emulation of a correct kernel, for the CPU tests)."""
    m = "fp16" if fault_here == "plain_fp16" else model
    if f32:
        mm = lambda a, c: (np.ascontiguousarray(a[:, ::-1], np.float32) @ np.ascontiguousarray(c[:, ::-1].T, np.float32)).astype(np.float64)
        bb = np.asarray(b, np.float32).astype(np.float64)
        fin = lambda y: np.asarray(y, np.float32).astype(np.float64)
    else:
        mm = lambda a, c: a @ c.T
        bb = np.asarray(b, np.float64)
        fin = lambda y: y
    if m == "split":
        xh, xl = split_parts(x)
        wh, wl = split_parts(w)
        if f32:
            return fin(fin(mm(xh, wh)) + fin(fin(mm(xh, wl) + mm(xl, wh)) / SPLIT) + bb)
        return xh @ wh.T + (xh @ wl.T + xl @ wh.T) / SPLIT + bb
    return fin(mm(_round(x, m), _round(w, m)) + bb)


def _act(y, model, fault_here=None):
    """ReLU output as the next layer's operand is formed from it (fp32 in the kernels' accumulators; the rounding happens in linear)"""
    y = np.maximum(y, 0.0)
    if fault_here == "rtz":
        return _rtz(y, model)
    return np.asarray(y, np.float32).astype(np.float64) if model != "exact" else y


def _bias(net, name, fault, layer):
    b = np.asarray(net[name], np.float64).copy()
    if fault is not None and fault[0] == "drop_bias" and fault[1] == layer:
        b[len(b) // 3] = 0.0
    return b


def _here(fault, layer):
    return fault[0] if fault is not None and fault[1] == layer else None


def sampling_mlp64(x, net0, model="exact", fault=None, f32=False):
    """The sampling network (src/models.py BaseNet: (depth - 1) x (Linear + ReLU) + Linear) -> [n, bins] float64."""
    n = len([k for k in net0 if k.endswith(".weight")])
    h = np.asarray(x, np.float32).astype(np.float64)
    for i in range(n):
        h = linear(h, net0["layers.%d.weight" % i], _bias(net0, "layers.%d.bias" % i, fault, i), model, _here(fault, i), f32)
        if i + 1 < n:
            h = _act(h, model, _here(fault, i))
    return h


def shading_mlp64(x, net1, n_pos, model="exact", fault=None, f32=False):
    """The shading network (src/models.py NeRF, any depth / skips) -> [n, 4] = (rgb, alpha) float64.  Layer indices of `fault`: the trunk's
    pts_linears.i are i; feature_linear is depth, views_linears.0 depth + 1, rgb_linear depth + 2."""
    x = np.asarray(x, np.float32).astype(np.float64)
    pts, views = x[:, :n_pos], x[:, n_pos:]
    depth = len([k for k in net1 if k.startswith("pts_linears.") and k.endswith(".weight")])
    width = net1["pts_linears.0.weight"].shape[0]
    skips = [i - 1 for i in range(1, depth) if net1["pts_linears.%d.weight" % i].shape[1] == width + n_pos]
    h = pts
    for i in range(depth):
        h = _act(linear(h, net1["pts_linears.%d.weight" % i], _bias(net1, "pts_linears.%d.bias" % i, fault, i), model, _here(fault, i), f32),
                 model, _here(fault, i))
        if i in skips:
            p = np.roll(pts, 1, axis=1) if _here(fault, i) == "skip_shift" else pts
            h = np.concatenate([p, h], axis=1)
    alpha = linear(h, net1["alpha_linear.weight"], net1["alpha_linear.bias"], model, None, f32)
    feat = linear(h, net1["feature_linear.weight"], _bias(net1, "feature_linear.bias", fault, depth), model, _here(fault, depth), f32)
    if model != "exact":
        feat = np.asarray(feat, np.float32).astype(np.float64)
    h = np.concatenate([feat, views], axis=1)
    h = _act(linear(h, net1["views_linears.0.weight"], _bias(net1, "views_linears.0.bias", fault, depth + 1), model, _here(fault, depth + 1),
                    f32), model, _here(fault, depth + 1))
    rgb = linear(h, net1["rgb_linear.weight"], net1["rgb_linear.bias"], model, _here(fault, depth + 2), f32)
    return np.concatenate([rgb, alpha], axis=1)


def pad_with_garbage(net, prefix, layer, value=0.05, seed=0):
    """The fault 'a padded column carrying a nonzero value': hidden width W (257..511) run as 512, where unit W of layer `layer` has
    bias `value` (its ReLU output is nonzero) and the next layer reads the padded columns with weights like the real ones."""
    rng = np.random.default_rng(seed)
    net = {k: v.copy() for k, v in net.items()}
    wn, bn = "%s%d.weight" % (prefix, layer), "%s%d.bias" % (prefix, layer)
    W = net[wn].shape[0]
    pad = 512 - W
    net[wn] = np.concatenate([net[wn], np.zeros((pad, net[wn].shape[1]), np.float32)])
    net[bn] = np.concatenate([net[bn], np.full(pad, value, np.float32)]).astype(np.float32)
    nx = "%s%d.weight" % (prefix, layer + 1)
    g = (rng.standard_normal((net[nx].shape[0], pad)) * np.sqrt(2.0 / W)).astype(np.float32)
    net[nx] = np.concatenate([net[nx], g], axis=1)      # the layer's own outputs are the last columns of the next layer's input
    return net


def sampling_hidden_max(x, net0):
    """per row: the largest input activation of any hidden layer of the sampling network (fp64): what has to stay inside the fp16 range"""
    n = len([k for k in net0 if k.endswith(".weight")])
    h = np.asarray(x, np.float32).astype(np.float64)
    m = np.zeros(h.shape[0])
    for i in range(n - 1):
        h = np.maximum(linear(h, net0["layers.%d.weight" % i], net0["layers.%d.bias" % i], "exact"), 0.0)
        m = np.maximum(m, h.max(axis=1))
    return m


def _cols(a):
    a = np.asarray(a, np.float64)
    return a.reshape(a.shape[0], -1)


def engine_errors(K, ref64, refq):
    """Per output column: the quantities check_engine bounds (also what the GPU tests log)."""
    K, ref64, refq = _cols(K), _cols(ref64), _cols(refq)
    scale = np.maximum(1.0, np.abs(ref64).max(axis=0))
    dq, d64, q64 = K - refq, K - ref64, refq - ref64
    rms = lambda d: np.sqrt(np.mean(d * d, axis=0))
    return dict(scale=scale, mean_z=np.abs(dq.mean(axis=0)) * np.sqrt(K.shape[0]) / np.maximum(rms(q64), 1e-300), rms_kq=rms(dq), rms_q64=rms(q64), max_kq=np.abs(dq).max(axis=0), max_q64=np.abs(q64).max(axis=0),
                max_k64=np.abs(d64).max(axis=0), finite=bool(np.isfinite(K).all()))


def check_engine(K, ref64, refq, engine, bounds=None, log=None):
    """Asserts that the output K of an MLP engine of class `engine` ("bf16", "fp16", "split", "fp32") agrees with its rounding model refq
    and with fp64 (ref64) within BOUNDS[engine] (or `bounds`), column by column.  log(summary) is called with the measured quantities before
    anything is asserted (conftest.record); the summary is also returned."""
    b = dict(BOUNDS[engine], **(bounds or {}))
    e = engine_errors(K, ref64, refq)
    out = dict(engine=engine, finite=e["finite"], max_k64_over_scale=float((e["max_k64"] / e["scale"]).max()))
    if engine in ("bf16", "fp16"):
        rms_ratio = e["rms_kq"] / np.maximum(e["rms_q64"], 1e-300)
        max_ratio = e["max_kq"] / np.maximum(e["max_q64"], 1e-300)
        out.update(rms_ratio=float(rms_ratio.max()), max_ratio=float(max_ratio.max()), mean_z=float(e["mean_z"].max()),
                   rms_q64=float(e["rms_q64"].min()))
    if log is not None:
        log(out)
    assert e["finite"], "%s: non-finite outputs" % engine
    if engine in ("bf16", "fp16"):
        c = int(np.argmax(rms_ratio))
        assert rms_ratio.max() <= b["rms_frac"], "%s: column %d: rms(K - model) = %.3g x rms(model - fp64) (bound %.3g)" % (
            engine, c, rms_ratio[c], b["rms_frac"])
        c = int(np.argmax(max_ratio))
        assert max_ratio.max() <= b["max_mult"], "%s: column %d: max|K - model| = %.3g x max|model - fp64| (bound %.3g)" % (
            engine, c, max_ratio[c], b["max_mult"])
        c = int(np.argmax(e["mean_z"]))
        assert e["mean_z"].max() <= b["mean_z"], "%s: column %d: systematic offset |mean(K - model)| sqrt(n) = %.3g x rms(model - fp64) (bound %.3g)" % (
            engine, c, e["mean_z"][c], b["mean_z"])
        lim = b["intrinsic"]
    else:
        lim = b["agree"]
    c = int(np.argmax(e["max_k64"] / e["scale"]))
    assert out["max_k64_over_scale"] <= lim, "%s: column %d: max|K - fp64| = %.3g (scale %.3g, bound %.3g x scale)" % (
        engine, c, e["max_k64"][c], e["scale"][c], lim)
    return out
