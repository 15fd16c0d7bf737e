"""Sampling networks whose raw outputs are exact by construction, so that the fused selection (pair_epilogue / pair_select inlined into the
sampling kernels, k_select_pair.hip.hpp) meets ties at the cut, the arg-max fallback, values equal to the threshold and non-finite rows on
whole frames -- rows that continuous (trained, Kaiming-random) networks never produce.  numpy only.

The construction (G gates; gate g reads one identity slot x_c of the encoding, never a sin / cos slot):
  layer 0, unit g     a_g = relu(1 - K (x_c - t_g)),  K = 64, t_g a quantile of column c over the frame the network is built for;
  layer 1             s_g = relu(1 - a_g): exactly 1 where a_g == 0, exactly 0 where a_g >= 1 -- in every engine (fp32, split fp16, plain
                      fp16), the only operands being 0, 1 and -1;
  middle layers       identity on the gate units (their place in the layer moves from layer to layer; every other weight and bias is 0);
  last layer          bias and the G weight columns are small multiples of 1/8 with many repeats: every output b + sum_g s_g w_g is a
                      dyadic number that fp16 holds and fp32 accumulation sums without rounding.
A ray is SATURATED when every gate's pre-activation 1 - K (x_c - t_g), in float64 on the ray's fp32 features, is <= -MARGIN or >= 1 + MARGIN;
its row is then b + W s with s in {0, 1}^G, bit for bit.  MARGIN = 0.25: the largest error of a pre-activation in any engine is the fp16
rounding of the input times K -- |x| <= 1, half an ulp 2^-12, times 64 = 2^-6 ~ 0.016 -- plus the rounding of the bias 1 + K t and a few ulp
of the device's own ray generation (1e-6 x 64); 0.25 is more than eight times that.  Rays inside a transition band carry general values.

overflow_gate: one more gate, on the second direction component, whose layer 1 is relu(4 - 4 a) (0 or 4, as exact as 0 or 1) and whose
layer-2 weight is 2^15 (fp16 holds it; 2^17 would already be inf as an operand): where it is open the hidden activation is 131 072 > 65 520, the smallest value that rounds to inf in fp16, so the split and plain-fp16 engines return a non-finite row there (the
fp16-range contract, adanerf_stats.sampling_overflow) while the fp32 engine returns the finite row (the gate's last-layer column is 0)."""
import dataclasses

import numpy as np

import adanerf_oracle as O

K = 64.0
MARGIN = 0.25
ABSENT = np.float32(-1e30)      # a depth cell the network does not have (multiDepthFeatures < 128): what the device pads its rows with
OVERFLOW_OPEN = 4.0             # layer-1 output of the open overflow gate
OVERFLOW_WEIGHT = 32768.0       # its layer-2 weight, 2^15: the hidden activation is 2^17


def identity_columns(scene):
    """columns of the sampling network's input that hold a raw direction component (0..2) and a raw position component (the next three
    identity slots): oracle_features is [PE(dir) | PE(pos)] and a positional encoding starts with x itself"""
    fp, fd = scene.pos_enc[0]
    return [0, 1, 2], [3 + 6 * fd + k for k in range(3)]


def gated_sampling_net(scene, feat, depth, width, bins, gates, seed, overflow_gate=False):
    """-> (net0 in the oracle's layout (layers.i.weight [out, in] / layers.i.bias, fp32), gate description).
    feat: the frame's features [n, scene.n_in0] (fp32), from which the gates' thresholds are taken; gates: G >= 3, spread over the three
    direction components.  The description: dict(col [G'], t [G'] float64 as stored (fp32 values), w_last [bins, G'] float64,
    b_last [bins] float64, overflow index or -1, bins) with G' = G + 1 under overflow_gate."""
    assert depth >= 3 and 1 <= bins <= 128 and 3 <= gates and gates + 1 <= width
    assert not overflow_gate or depth >= 4, "the overflow gate needs a hidden layer 2"
    rng = np.random.default_rng(seed)
    feat = np.asarray(feat, np.float32)
    n_in = feat.shape[1]
    assert n_in == scene.n_in0
    dir_cols, _ = identity_columns(scene)
    col = np.array([dir_cols[g % 3] for g in range(gates)])
    # quantiles spread over (0.12, 0.88), different per gate so that the gate edges cross the image at different places
    qs = 0.12 + 0.76 * (np.arange(gates) + 0.5) / gates
    qs = qs[rng.permutation(gates)]
    t = np.array([np.quantile(feat[:, c].astype(np.float64), q) for c, q in zip(col, qs)])
    if overflow_gate:
        col = np.append(col, dir_cols[1])
        t = np.append(t, np.quantile(feat[:, dir_cols[1]].astype(np.float64), 0.5))
    G = col.size
    t = t.astype(np.float32).astype(np.float64)
    # where the gate units sit in each hidden layer: spread over the width, first and last unit included, moved from layer to layer
    place = []
    for i in range(depth - 1):
        p = np.unique(np.round(np.linspace(0, width - 1, G)).astype(np.int64))
        assert p.size == G
        place.append(np.roll(p, i)[rng.permutation(G)] if i else p)
    net = {}
    dims = [n_in] + [width] * (depth - 1) + [bins]
    for i in range(depth):
        net["layers.%d.weight" % i] = np.zeros((dims[i + 1], dims[i]), np.float32)
        net["layers.%d.bias" % i] = np.zeros(dims[i + 1], np.float32)
    net["layers.0.weight"][place[0], col] = -K
    net["layers.0.bias"][place[0]] = (1.0 + K * t).astype(np.float32)
    net["layers.1.weight"][place[1], place[0]] = -1.0
    net["layers.1.bias"][place[1]] = 1.0
    for i in range(2, depth - 1):
        net["layers.%d.weight" % i][place[i], place[i - 1]] = 1.0
    # the last layer: multiples of 1/8, few distinct values, 30 % of the weights non-zero
    b_last = rng.integers(-2, 3, bins) / 8.0
    w_last = rng.integers(1, 4, (bins, G)) / 8.0 * (rng.random((bins, G)) < 0.3) * np.where(rng.random((bins, G)) < 0.25, -1.0, 1.0)
    ov = -1
    if overflow_gate:
        ov = G - 1
        w_last[:, ov] = 0.0
        net["layers.1.weight"][place[1][ov], place[0][ov]] = -OVERFLOW_OPEN
        net["layers.1.bias"][place[1][ov]] = OVERFLOW_OPEN
        net["layers.2.weight"][place[2][ov], place[1][ov]] = OVERFLOW_WEIGHT
    net["layers.%d.weight" % (depth - 1)][:, place[depth - 2]] = w_last.astype(np.float32)
    net["layers.%d.bias" % (depth - 1)][:] = b_last.astype(np.float32)
    return net, dict(col=col, t=t, w_last=w_last, b_last=b_last, overflow=ov, bins=bins)


def gate_preactivations(feat, gates):
    """1 - K (x_c - t_g) per ray and gate, float64 on the fp32 features"""
    x = np.asarray(feat, np.float32).astype(np.float64)[:, gates["col"]]
    return 1.0 - K * (x - gates["t"][None, :])


def predict(feat64, gates, engine16=False):
    """-> (saturated [n] bool at MARGIN, rows [n, 128] float64: b + W s on saturated rays (cells past `bins` at ABSENT), NaN elsewhere).
    engine16: the row a split / plain-fp16 engine returns -- all NaN where the overflow gate is open (non-finite; the test compares
    finiteness there, not bits)."""
    z = gate_preactivations(feat64, gates)
    sat = ((z <= -MARGIN) | (z >= 1.0 + MARGIN)).all(axis=1)
    s = (z <= -MARGIN).astype(np.float64)      # a_g == 0  <=>  the gate is open
    rows = np.full((z.shape[0], 128), float(ABSENT))
    rows[:, :gates["bins"]] = gates["b_last"][None, :] + s @ gates["w_last"].T
    rows[~sat] = np.nan
    if engine16 and gates["overflow"] >= 0:
        rows[sat & (s[:, gates["overflow"]] == 1.0)] = np.nan
    return sat, rows


def overflow_open(feat64, gates):
    """rays on which the overflow gate is saturated open (the engines with fp16 operands return a non-finite row there)"""
    z = gate_preactivations(feat64, gates)
    return z[:, gates["overflow"]] <= -MARGIN if gates["overflow"] >= 0 else np.zeros(z.shape[0], bool)


def classes(rows, N, thr):
    """per-ray flags of the selection's difficult rows, on fp32 rows [n, 128]:
    tie       a tie at the cut: #(x >= max(v_N, thr)) > N (v_N the N-th largest value);
    fallback  nothing reaches the threshold: max < thr (the arg-max alone is kept);
    at_thr    a value == thr among the N largest;
    nonfinite a NaN or an infinity in the row;
    max_tie   a fallback row whose maximum occurs more than once (the tie rule with a budget of one)."""
    x = np.asarray(rows, np.float32)
    thr = np.float32(thr)
    with np.errstate(invalid="ignore"):
        srt = -np.sort(-x, axis=1)
        vn = srt[:, N - 1]
        cut = np.maximum(vn, thr)
        fallback = srt[:, 0] < thr
        return dict(tie=(x >= cut[:, None]).sum(axis=1) > N, fallback=fallback, at_thr=(srt[:, :N] == thr).any(axis=1),
                    nonfinite=~np.isfinite(x).all(axis=1), max_tie=fallback & ((x == srt[:, :1]).sum(axis=1) > 1))


def mixed_blocks(flag, valid=None, block=32):
    """number of blocks of `block` consecutive rays (one wave's rays) that hold both a flagged ray and an unflagged one; rays with
    valid == False count as neither"""
    flag = np.asarray(flag, bool)
    valid = np.ones_like(flag) if valid is None else np.asarray(valid, bool)
    n = -(-flag.size // block) * block
    f = np.zeros(n, bool)
    g = np.zeros(n, bool)
    f[:flag.size] = flag & valid
    g[:flag.size] = ~flag & valid
    return int((f.reshape(-1, block).any(axis=1) & g.reshape(-1, block).any(axis=1)).sum())


def brute_force_select(row, N, thr):
    """the rule in three lines: the bins of the values >= thr, by value descending and bin ascending, the first N of them -- or the first
    arg-max; ascending"""
    order = sorted(range(len(row)), key=lambda b: (-row[b], b))
    kept = [b for b in order if row[b] >= thr][:N] or order[:1]
    return sorted(kept)


# ---- the models and the walk both test files use -------------------------------------------------------------------------------------------

W, H = 97, 61      # 5 917 rays: ragged 32- / 128- / 256-ray tiles
GATES = 6
# name: depth, width, encoding of the sampling net, depth cells, seed, overflow gate.  8 x 256 with 10-4 / 2-2 are the fixed kernels' two
# instantiations; everything else runs the run-time-shaped kernel ((6, 3) is packed into the 16-band catch-all layout).  The seeds are
# chosen so that the class floors of tests/test_tie_networks_cpu.py hold; that file is where a change of the construction shows.
MODELS = {
    "fixed_10_4": dict(depth=8, width=256, pe0=(10, 4), bins=128, seed=1, overflow=False),
    "fixed_2_2": dict(depth=8, width=256, pe0=(2, 2), bins=128, seed=2, overflow=False),
    "gen_4x64_catchall": dict(depth=4, width=64, pe0=(6, 3), bins=128, seed=3, overflow=False),
    "gen_6x128_bins100": dict(depth=6, width=128, pe0=(10, 4), bins=100, seed=11, overflow=False),
    "gen_5x256": dict(depth=5, width=256, pe0=(10, 4), bins=128, seed=5, overflow=False),
    "fixed_10_4_overflow": dict(depth=8, width=256, pe0=(10, 4), bins=128, seed=1, overflow=True),
    "gen_6x128_overflow": dict(depth=6, width=128, pe0=(10, 4), bins=128, seed=6, overflow=True),
}
PLAIN = [m for m in MODELS if not MODELS[m]["overflow"]]
OVERFLOW = [m for m in MODELS if MODELS[m]["overflow"]]
# (N, thr, kind): N over the pair_select<4 | 8 | 16> boundaries; thr "equal" to a row value (1/8: below the N largest of most rows; 1/2:
# among them), "between" two row values, "above" every row value (every ray falls back to its arg-max; a repeated maximum is a tie there)
WALK = ([(n, t, "equal") for t in (0.125, 0.5) for n in (1, 2, 3, 4, 5, 8, 11, 16)] + [(n, 0.5625, "between") for n in (1, 2, 4, 5, 8)] +
        [(n, 4.0, "above") for n in (1, 3, 11, 16)])
FLOORS = dict(tie=0.10, fallback=0.03, tie_blocks=20, fallback_blocks=10, saturated=0.50, distinct=8)


def frame_features(scene, pose, rot, w, h):
    """the sampling network's inputs for a w x h frame, as the oracle computes them (fp32)"""
    nds, p = O.world_rays(O.generate_ray_directions(w, h, scene.fov), pose, rot, scene)
    return O.oracle_features(nds, p, scene)


def build(name, base_case):
    """-> (scene, O.Weights, gates, features of the W x H frame) of MODELS[name]; base_case = conftest.load_case("synthetic_fixed8").  The
    gates' thresholds are quantiles over the W x H frame; any other frame size with this camera sees the same field of view."""
    z, meta, sc = base_case
    m = MODELS[name]
    sc = dataclasses.replace(sc, pos_enc=(tuple(m["pe0"]), sc.pos_enc[1]), depth_bins=m["bins"])
    feat = frame_features(sc, z["pose"], z["rot"], W, H)
    net0, gates = gated_sampling_net(sc, feat, m["depth"], m["width"], m["bins"], GATES, m["seed"], overflow_gate=m["overflow"])
    return sc, O.Weights(net0, O.synthetic_weights(900 + m["seed"]).net1), gates, feat


def pad_rows(rows, dtype=np.float32):
    """[n, bins] network outputs -> [n, 128] device rows (absent cells at ABSENT)"""
    rows = np.asarray(rows)
    out = np.full((rows.shape[0], 128), ABSENT, dtype)
    out[:, :rows.shape[1]] = rows
    return out


def class_counts(rows, sat, n, thr):
    """what the floors are stated on, for one (N, thr): shares of all rays and numbers of 32-ray blocks; only saturated rays count as tie /
    fallback rays (their rows are known in advance), every ray counts on the other side of a mixed block"""
    c = classes(rows, n, thr)
    tie, fb, mt = c["tie"] & sat, c["fallback"] & sat, c["max_tie"] & sat
    return dict(tie=float(tie.mean()), fallback=float(fb.mean()), at_thr=float((c["at_thr"] & sat).mean()), max_tie=float(mt.mean()),
                nonfinite=int(c["nonfinite"].sum()), tie_blocks=mixed_blocks(tie), fallback_blocks=mixed_blocks(fb), max_tie_blocks=mixed_blocks(mt))


def check_floors(counts_by_pair, what):
    """the conditions of the issue on the classes reached (counts_by_pair: {(N, thr, kind): class_counts}); asserts, never skips"""
    for (n, thr, kind), c in counts_by_pair.items():
        if kind == "above":      # every saturated ray falls back; the tie rule runs with a budget of one on the repeated maxima
            assert c["max_tie"] >= FLOORS["tie"] and c["max_tie_blocks"] >= FLOORS["tie_blocks"], (what, n, thr, c)
        else:
            assert c["tie"] >= FLOORS["tie"] and c["tie_blocks"] >= FLOORS["tie_blocks"], (what, n, thr, c)
    assert any(c["fallback"] >= FLOORS["fallback"] and c["fallback_blocks"] >= FLOORS["fallback_blocks"] for (n, t, k), c in counts_by_pair.items()
               if k != "above"), (what, "no pair with mixed fallback blocks")
    assert any(c["at_thr"] >= FLOORS["tie"] for c in counts_by_pair.values()), (what, "no pair with values equal to the threshold")
