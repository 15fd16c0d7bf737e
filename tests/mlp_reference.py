"""fp64 evaluation of the two networks under explicit rounding models, and the comparator every MLP engine test uses.

Networks come as the oracle's weight dicts (``O.Weights.net0`` / ``.net1``), inputs as fp32 feature rows.  Rounding models:

- ``exact``: fp64 throughout.
- ``bf16`` / ``fp16``: every operand of a matrix product is rounded to the MFMA operand type (RNE, ``mfma_emulation.quantize``): the
  weights, the encoded inputs (identity slots included), every ReLU output, the skip concatenation (which reuses the rounded
  encoding) and ``feature_linear``'s output feeding ``views_linears.0``.  Biases and accumulation stay exact.  The bf16 packer's
  per-layer powers of two (pack.cpp scale_layer) commute with every rounding on the way and are not modelled; ``rescale`` below builds
  the networks that put exactly that under test (tests/test_shading_ranges_cpu.py, tests/test_gpu_shading_ranges.py).
- ``split``: every operand is ``hi + 2^-11 lo'`` with both parts fp16 (pack.cpp F16_SPLIT, k_sampling16.hip.hpp split_pack), and a
  product keeps ``hi*hi + hi*lo' + lo'*hi`` (the ``lo'*lo'`` term, 2^-22 relative, is dropped as the kernels drop it).

Faults (``fault=(kind, layer)``) are the emulated kernel bugs the CPU suite shows the comparator rejects (tests/test_mlp_reference_cpu.py).
``("clamp", layer, e)``: the ReLU output of that layer is cut at 2^(e - 1), half the power of two 2^e the bf16 packer chose for it
(mfma_emulation.scale_exponents): what the kernels' clamped conversion does to a layer whose scale exponent came out one too small.
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


def _act(y, model, fault_here=None, cut=None):
    """ReLU output as the next layer's operand is formed from it (fp32 in the kernels' accumulators; the rounding happens in linear)"""
    y = np.maximum(y, 0.0)
    if fault_here == "rtz":
        return _rtz(y, model)
    if fault_here == "clamp":
        y = np.minimum(y, cut)
    return np.asarray(y, np.float32).astype(np.float64) if model != "exact" else y


def _bias(net, name, fault, layer):
    b = np.asarray(net[name], np.float64).copy()
    if fault is not None and fault[0] == "drop_bias" and fault[1] == layer:
        b[len(b) // 3] = 0.0
    return b


def _here(fault, layer):
    return fault[0] if fault is not None and fault[1] == layer else None


def _cut(fault):
    """("clamp", layer, e): the value the layer's ReLU output is cut at, 2^(e - 1)"""
    return float(np.ldexp(1.0, int(fault[2]) - 1)) if fault is not None and fault[0] == "clamp" else None


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
                 model, _here(fault, i), _cut(fault))
        if i in skips:
            p = np.roll(pts, 1, axis=1) if _here(fault, i) == "skip_shift" else pts
            h = np.concatenate([p, h], axis=1)
    alpha = linear(h, net1["alpha_linear.weight"], net1["alpha_linear.bias"], model, None, f32)
    feat = linear(h, net1["feature_linear.weight"], _bias(net1, "feature_linear.bias", fault, depth), model, _here(fault, depth), f32)
    if model != "exact":
        feat = np.asarray(feat, np.float32).astype(np.float64)
    h = np.concatenate([feat, views], axis=1)
    h = _act(linear(h, net1["views_linears.0.weight"], _bias(net1, "views_linears.0.bias", fault, depth + 1), model, _here(fault, depth + 1),
                    f32), model, _here(fault, depth + 1), _cut(fault))
    rgb = linear(h, net1["rgb_linear.weight"], net1["rgb_linear.bias"], model, _here(fault, depth + 2), f32)
    return np.concatenate([rgb, alpha], axis=1)


def shading_layer_names(net1):
    """the shading net's layers in the order of `rescale`'s exponents: the trunk, then feature_linear, alpha_linear, views_linears.0, rgb_linear"""
    depth = len([k for k in net1 if k.startswith("pts_linears.") and k.endswith(".weight")])
    return ["pts_linears.%d" % i for i in range(depth)] + ["feature_linear", "alpha_linear", "views_linears.0", "rgb_linear"]


def rescale(net1, n_pos, E):
    """The shading network with the OUTPUT of every layer times 2^E[layer] (E: one integer per layer, in shading_layer_names order).  ReLU is
    positively homogeneous, so it is enough to multiply every weight column block by 2^(E_layer - E_source) -- E_source is the exponent of the
    layer the columns read, 0 for encoding columns (layer 0, the skip concatenation, the direction columns of views_linears.0) -- and every
    bias by 2^E_layer.  The layers without an activation take their own E like the others.  In real arithmetic the result is the base network
    with alpha times 2^Ea and rgb times 2^Ec (Ea = E[alpha_linear], Ec = E[rgb_linear]); in fp32 every factor is an exact power of two, and the
    function refuses a schedule under which a weight or bias would leave fp32's normal range (the scaling would round)."""
    names = shading_layer_names(net1)
    depth = len(names) - 4
    E = [int(e) for e in E]
    assert len(E) == len(names), (len(E), names)
    e_of = dict(zip(names, E))
    width = net1["pts_linears.0.weight"].shape[0]

    def scaled(a, k):
        a = np.asarray(a, np.float32)
        out = np.ldexp(a, k).astype(np.float32)
        nz = a != 0
        assert np.isfinite(out).all() and (np.abs(out[nz]) >= np.finfo(np.float32).tiny).all(), "rescale: 2^%s leaves fp32's normal range" % (k,)
        return out

    out = {}
    for i in range(depth):
        nm = "pts_linears.%d" % i
        w = np.asarray(net1[nm + ".weight"], np.float32)
        e, src = e_of[nm], (e_of["pts_linears.%d" % (i - 1)] if i else 0)
        if i == 0:
            cols = np.full(w.shape[1], e, np.int64)                     # encoding columns only
        elif w.shape[1] == width + n_pos:
            cols = np.concatenate([np.full(n_pos, e, np.int64), np.full(width, e - src, np.int64)])      # cat([input_pts, h])
        else:
            cols = np.full(w.shape[1], e - src, np.int64)
        out[nm + ".weight"] = scaled(w, cols[None, :])
        out[nm + ".bias"] = scaled(net1[nm + ".bias"], e)
    eh, ef, ev = e_of["pts_linears.%d" % (depth - 1)], e_of["feature_linear"], e_of["views_linears.0"]
    for nm, src in (("feature_linear", eh), ("alpha_linear", eh), ("rgb_linear", ev)):
        out[nm + ".weight"] = scaled(net1[nm + ".weight"], e_of[nm] - src)
        out[nm + ".bias"] = scaled(net1[nm + ".bias"], e_of[nm])
    w = np.asarray(net1["views_linears.0.weight"], np.float32)
    cols = np.concatenate([np.full(width, ev - ef, np.int64), np.full(w.shape[1] - width, ev, np.int64)])      # cat([feature, input_views])
    out["views_linears.0.weight"] = scaled(w, cols[None, :])
    out["views_linears.0.bias"] = scaled(net1["views_linears.0.bias"], ev)
    assert set(out) == set(net1)
    return out


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


def shading_hidden_max(x, net1, n_pos):
    """the largest trunk activation of the shading network over all rows (fp64): what an fp16 engine would have to hold"""
    x = np.asarray(x, np.float32).astype(np.float64)
    pts = x[:, :n_pos]
    depth = len([k for k in net1 if k.startswith("pts_linears.") and k.endswith(".weight")])
    width = net1["pts_linears.0.weight"].shape[0]
    h, m = pts, 0.0
    for i in range(depth):
        w = net1["pts_linears.%d.weight" % i]
        if i and w.shape[1] == width + n_pos:
            h = np.concatenate([pts, h], axis=1)
        h = np.maximum(linear(h, w, net1["pts_linears.%d.bias" % i], "exact"), 0.0)
        m = max(m, float(h.max()))
    return m


def emulation_bounds(x, net1, n_pos, engine, ref64, refq):
    """check_engine bounds for a 16-bit engine on rows whose errors are not the Kaiming nets' errors (positions far from the origin, other
    normalisations): per quantity the larger of BOUNDS[engine] and 1.5 x what the emulated correct kernel (f32=True: the model's operands,
    fp32 products summed in another order) shows on the same rows.  Computed from the reference alone, never from a kernel's output.
    Returns (bounds, shown)."""
    emu = shading_mlp64(x, net1, n_pos, engine, f32=True)
    e = engine_errors(emu, ref64, refq)
    shown = dict(rms_frac=float((e["rms_kq"] / np.maximum(e["rms_q64"], 1e-300)).max()),
                 max_mult=float((e["max_kq"] / np.maximum(e["max_q64"], 1e-300)).max()), mean_z=float(e["mean_z"].max()),
                 intrinsic=float((e["max_k64"] / e["scale"]).max()))
    return {k: max(BOUNDS[engine][k], 1.5 * v) for k, v in shown.items()}, shown


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
