"""Networks whose outputs ARE chosen input slots, exact in every engine, so that the positional encoding every fused MLP kernel computes for
itself (pe_eval<F, ACCURATE> / pe_pack / pe_eval_wide) can be read slot by slot -- tests/tie_networks.py reads "never a sin / cos slot", and
trained or random networks pass a wrong slot on as a few percent of RMS error.  numpy only; the form is tie_networks': weights in {0, +1, -1},
all biases 0.

Sampling probe (depth, width, up to min(128, width // 2) columns of the input):
  layer 0             u+_j = relu(f_j), u-_j = relu(-f_j) for every probed column j;
  middle layers       identity on those 2 k units (their place in the layer moves from layer to layer; every other weight is 0);
  last layer          out_j = u+_j - u-_j.
Shading probe (depth, width, skips, four columns): one position column goes through the trunk (u+, u-) to alpha_linear; three columns go to
rgb_linear through views_linears.0 (v+, v-) -- direction columns enter there, position columns are carried through the trunk and come out of
feature_linear as u+ - u-.  Skip columns are zero.
Every sum has one non-zero term, so the output is the engine's operand rounding of the slot and nothing else (ROUNDING below; the CPU test
shows it equals mlp_reference's models bit for bit): fp32 keeps the bits, bf16 / fp16 round once (the later layers see a 16-bit value), the
split engine keeps hi + 2^-11 lo'.

expected(): the slot values in float64, in the oracle's column order [x, sin 2^0 x, cos 2^0 x, ...], in two forms:
  "accurate"   sin / cos of the exact product x 2^b (what sin_or_cos approximates);
  "fast"       sin(2 pi r32), r32 = fp32(a fp32(1 / 2 pi) + q) with ONE rounding, q = 0.25 for the cosine: the exact value of what
               pe_eval's !ACCURATE arm hands to v_sin_f32, whose input is in revolutions.
check_slots(): rounding is monotone, so a slot the device computed within E of s comes out of the probe between ROUNDING(s - E) and
ROUNDING(s + E); identity slots have E = 0.  No bound here is fitted to a kernel's output; of the inputs, only the depths of the
raySampleInput points are read off the device (fit_ray_sample_depths: from the debug kernel's identity columns, exactly or not at all).

The scenes (near / far / straddle) and what each has to put in front of the kernels (conditions) are here too, so that the CPU test and the
GPU test state them on the same code."""
import dataclasses
import math

import numpy as np

import adanerf_oracle as O
import mlp_reference as M
from mfma_emulation import quantize

W, H = 97, 61      # 5 917 rays: 47 tiles of 128 with a ragged last one, no multiple of 32, 64 or 256
N_SHADE = 2570     # samples the shading probes run on (as tests/test_gpu_shading_ranges.py)
INV_2PI_F32 = np.float32(0.15915494309189535)      # the constant of pe_eval's !ACCURATE arm, rounded to fp32 as the compiler rounds it
E_ACCURATE_SMALL, E_ACCURATE_LARGE = 1.2e-7, 2e-7      # the stated accuracy of sin_or_cos (test_device_sin_or_cos_accuracy): |a| < 1e5, beyond
E_FAST = 2.0 ** -18      # v_sin_f32 on an exact fp32 revolution count: 64 fp32 ulp at 1.0, 1 / 64 of the fp16 half-ulp at 1.0
REV_LIMIT = 256.0        # the documented domain of V_SIN_F32, in revolutions
SMALL_LIMIT = 1.0e5      # pe_eval's wave-uniform range test, in radians


# ---- columns ------------------------------------------------------------------------------------------------------------------------------

def pe_columns(F):
    """[(kind, band, component)] of the 3 + 6 F columns of O.positional_encoding: kind "id" (band -1), "sin" or "cos" """
    cols = [("id", -1, c) for c in range(3)]
    for b in range(F):
        cols += [("sin", b, c) for c in range(3)] + [("cos", b, c) for c in range(3)]
    return cols


def sampling_columns(scene):
    """[(block, F, kind, band, component)] of the sampling network's input: block 0 = PE(direction), 1 = PE(position), 2.. = the
    raySampleInput points (O.oracle_features)"""
    fp, fd = scene.pos_enc[0]
    cols = [(0, fd) + c for c in pe_columns(fd)] + [(1, fp) + c for c in pe_columns(fp)]
    for a in range(scene.ray_sample_input):
        cols += [(2 + a, fp) + c for c in pe_columns(fp)]
    assert len(cols) == scene.n_in0
    return cols


def shading_columns(scene):
    """the same for the shading network: block 0 = PE(position), 1 = PE(direction) (O.shading_inputs)"""
    fp, fd = scene.pos_enc[1]
    return [(0, fp) + c for c in pe_columns(fp)] + [(1, fd) + c for c in pe_columns(fd)]


# ---- the probes ---------------------------------------------------------------------------------------------------------------------------

def _places(rng, n_layers, width, units):
    """where `units` carried units sit in each of n_layers hidden layers: spread over the width, first and last unit included, moved from layer
    to layer (tie_networks.gated_sampling_net)"""
    p = np.unique(np.round(np.linspace(0, width - 1, units)).astype(np.int64))
    assert p.size == units, (width, units)
    return [np.roll(p, i)[rng.permutation(units)] if i else p for i in range(n_layers)]


def sampling_probe(n_in, depth, width, slots, seed=0, bins=128, sign=1.0):
    """-> net0 in the oracle's layout (fp32) whose output j is input column slots[j] (sign = -1: its negative, exact as well, so that a
    selection that keeps the largest values sees the negative slots); outputs past len(slots) are 0"""
    slots = np.asarray(slots, np.int64)
    k = slots.size
    assert depth >= 2 and 1 <= k <= min(128, width // 2) and k <= bins and len(set(slots.tolist())) == k and slots.max() < n_in
    rng = np.random.default_rng(seed)
    place = _places(rng, depth - 1, width, 2 * k)
    dims = [n_in] + [width] * (depth - 1) + [bins]
    net = {}
    for i in range(depth):
        net["layers.%d.weight" % i] = np.zeros((dims[i + 1], dims[i]), np.float32)
        net["layers.%d.bias" % i] = np.zeros(dims[i + 1], np.float32)
    net["layers.0.weight"][place[0][:k], slots] = 1.0
    net["layers.0.weight"][place[0][k:], slots] = -1.0
    for i in range(1, depth - 1):
        net["layers.%d.weight" % i][place[i], place[i - 1]] = 1.0
    last = net["layers.%d.weight" % (depth - 1)]
    last[np.arange(k), place[depth - 2][:k]] = sign
    last[np.arange(k), place[depth - 2][k:]] = -sign
    return net


def slot_groups(n_in, width):
    """the input columns in as few sampling probes as the width carries: min(128, width // 2) columns each"""
    per = min(128, width // 2)
    return [list(range(i, min(n_in, i + per))) for i in range(0, n_in, per)]


def shading_probe(n_pos, n_dir, depth, width, skips, slots, seed=0):
    """-> net1 in the oracle's layout whose outputs (r, g, b, alpha) are the input columns slots = (a, c0, c1, c2) of [PE(pos) | PE(dir)]:
    a < n_pos goes through the trunk to alpha_linear; c_k < n_pos is carried through the trunk and feature_linear, c_k >= n_pos enters at
    views_linears.0"""
    a, cs = int(slots[0]), [int(c) for c in slots[1:]]
    assert len(cs) == 3 and 0 <= a < n_pos and all(0 <= c < n_pos + n_dir for c in cs) and depth >= 1 and width >= 16
    rng = np.random.default_rng(seed)
    carried = [a] + [c for c in cs if c < n_pos]      # position columns that ride the trunk, as (u+, u-) pairs
    k = len(carried)
    place = _places(rng, depth, width, 2 * k)
    net = {}
    for i in range(depth):
        n_k = n_pos if i == 0 else (width + n_pos if (i - 1) in skips else width)
        net["pts_linears.%d.weight" % i] = np.zeros((width, n_k), np.float32)
        net["pts_linears.%d.bias" % i] = np.zeros(width, np.float32)
    for nm, (o, n_k) in {"views_linears.0": (width // 2, width + n_dir), "feature_linear": (width, width), "alpha_linear": (1, width),
                         "rgb_linear": (3, width // 2)}.items():
        net[nm + ".weight"] = np.zeros((o, n_k), np.float32)
        net[nm + ".bias"] = np.zeros(o, np.float32)
    net["pts_linears.0.weight"][place[0][:k], carried] = 1.0
    net["pts_linears.0.weight"][place[0][k:], carried] = -1.0
    for i in range(1, depth):
        off = n_pos if (i - 1) in skips else 0      # cat([input_pts, h]): the skip columns stay zero
        net["pts_linears.%d.weight" % i][place[i], off + place[i - 1]] = 1.0
    top = place[depth - 1]
    net["alpha_linear.weight"][0, top[0]] = 1.0
    net["alpha_linear.weight"][0, top[k]] = -1.0
    fplace = _places(rng, 1, width, 3)[0]            # feature_linear's outputs: the carried colour columns, u+ - u-
    vplace = _places(rng, 1, width // 2, 6)[0]       # views_linears.0: v+_k at vplace[k], v-_k at vplace[3 + k]
    for kk, c in enumerate(cs):
        if c < n_pos:
            j = 1 + sum(1 for x in cs[:kk] if x < n_pos)      # its own (u+, u-) pair, also where it repeats another column
            net["feature_linear.weight"][fplace[kk], top[j]] = 1.0
            net["feature_linear.weight"][fplace[kk], top[k + j]] = -1.0
            src = fplace[kk]
        else:
            src = width + (c - n_pos)                # cat([feature, input_views])
        net["views_linears.0.weight"][vplace[kk], src] = 1.0
        net["views_linears.0.weight"][vplace[3 + kk], src] = -1.0
        net["rgb_linear.weight"][kk, vplace[kk]] = 1.0
        net["rgb_linear.weight"][kk, vplace[3 + kk]] = -1.0
    return net


def shading_plan(n_pos, n_dir):
    """[(a, c0, c1, c2)]: the fewest probes that read every column -- 23 for the 63 + 27 columns of the 10-4 encoding.  alpha takes position
    columns from the front, the colours take the rest in order (position columns first, then the direction columns), wrapping at the end."""
    total = n_pos + n_dir
    n = next(n for n in range(1, total + 1) if min(n, n_pos) + 3 * n >= total)
    alphas = [i % n_pos for i in range(n)]
    rest = [c for c in range(total) if c not in set(alphas)]
    plan = [(alphas[i],) + tuple(rest[(3 * i + j) % len(rest)] for j in range(3)) for i in range(n)]
    assert {c for p in plan for c in p} == set(range(total))
    return plan


# ---- what the slots are -------------------------------------------------------------------------------------------------------------------

def _fma_f32(a32, c32, q32):
    """fp32(a c + q) with one rounding: the product of two fp32 is exact in float64; the sum is rounded to odd there (TwoSum tells whether it
    was exact), which makes the final rounding to fp32 the rounding of the exact sum"""
    p = a32.astype(np.float64) * np.float64(c32)
    q = np.broadcast_to(np.float64(q32), p.shape)
    s = p + q
    bb = s - p
    err = (p - (s - bb)) + (q - bb)
    bits = s.view(np.int64) if s.flags["C_CONTIGUOUS"] else np.ascontiguousarray(s).view(np.int64)
    even = (bits & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def arguments(x32, F):
    """the exact arguments a = x 2^b, float64 [n, F, 3]"""
    x = np.asarray(x32, np.float32).astype(np.float64)
    return x[:, None, :] * (2.0 ** np.arange(F))[None, :, None]


def revolutions(x32, F):
    """|a| / 2 pi, [n, F, 3]"""
    return np.abs(arguments(x32, F)) / (2.0 * math.pi)


def expected(x32, F, form):
    """x32 [n, 3]: the device's own fp32 x -> float64 [n, 3 + 6 F] slot values in the order of O.positional_encoding"""
    x32 = np.ascontiguousarray(x32, np.float32)
    a = arguments(x32, F)
    if form == "accurate":
        sn, cs = np.sin(a), np.cos(a)
    else:
        assert form == "fast", form
        a32 = a.astype(np.float32)
        assert (a32.astype(np.float64) == a).all()      # x 2^b is exact in fp32 too
        turn = lambda r32: np.sin(2.0 * math.pi * (r32.astype(np.float64) - np.rint(r32.astype(np.float64))))
        sn = turn(_fma_f32(a32, INV_2PI_F32, np.float32(0.0)))
        cs = turn(_fma_f32(a32, INV_2PI_F32, np.float32(0.25)))
    out = np.empty((x32.shape[0], 3 + 6 * F))
    out[:, :3] = x32
    for b in range(F):
        out[:, 3 + 6 * b:6 + 6 * b] = sn[:, b]
        out[:, 6 + 6 * b:9 + 6 * b] = cs[:, b]
    return out


def widening(x32, F, form):
    """E per column [n, 3 + 6 F]: 0 on the identity columns; accurate: 1.2e-7 where |a| < 1e5 and 2e-7 beyond; fast: 2^-18"""
    a = np.abs(arguments(x32, F))
    e = np.where(a < SMALL_LIMIT, E_ACCURATE_SMALL, E_ACCURATE_LARGE) if form == "accurate" else np.full(a.shape, E_FAST)
    out = np.zeros((a.shape[0], 3 + 6 * F))
    for b in range(F):
        out[:, 3 + 6 * b:6 + 6 * b] = e[:, b]
        out[:, 6 + 6 * b:9 + 6 * b] = e[:, b]
    return out


def ROUNDING(v, model):
    """what a probe returns for a slot of value v under mlp_reference's model `model` ("exact" stands for the fp32 engines: the bits of
    fp32(v)); float64 in, float64 out, monotone"""
    v32 = np.asarray(v, np.float64).astype(np.float32)
    if model == "exact":
        return v32.astype(np.float64)
    if model == "bf16":
        return quantize(v32, 0).astype(np.float64)
    if model == "fp16":
        return quantize(v32, 1).astype(np.float64)
    assert model == "split", model
    hi, lo = M.split_parts(v32)
    return hi + lo / M.SPLIT


def check_slots(out, s, E, model, bands=None, truth=None, probe=None):
    """out [n, k]: what the probes returned for k columns; s, E [n, k]: their expected values and widenings; model: "exact" | "split" |
    "fp16" | "bf16".  -> dict(bad [n, k] bool: out outside [ROUNDING(s - E), ROUNDING(s + E)] or not finite; moved [n, k] bool: out differs
    from ROUNDING(s); per_band {band: dict(slots, bad, moved share, max_err)} with bands [k] (-1 = identity) and truth [n, k] = sin64(a):
    max_err is max |out - truth|).
    probe: a callable features -> outputs (mlp_reference on a real probe network); the three bounds are then taken from it, not from
    ROUNDING -- the CPU test shows that the two are the same numbers."""
    out = np.asarray(out, np.float64)
    s, E = np.asarray(s, np.float64), np.broadcast_to(np.asarray(E, np.float64), np.shape(s))
    assert out.shape == s.shape and (E >= 0).all()
    f = probe if probe is not None else (lambda v: ROUNDING(v, model))
    lo, mid, hi = f(s - E), f(s), f(s + E)
    with np.errstate(invalid="ignore"):
        bad = ~((out >= lo) & (out <= hi))
    moved = out != mid
    res = dict(bad=bad, moved=moved, per_band={})
    if bands is not None:
        bands = np.asarray(bands)
        truth = s if truth is None else np.asarray(truth, np.float64)
        for b in np.unique(bands):
            m = bands == b
            res["per_band"][int(b)] = dict(slots=int(m.sum()) * out.shape[0], bad=int(bad[:, m].sum()), moved=float(moved[:, m].mean()),
                                           max_err=float(np.nanmax(np.abs(out[:, m] - truth[:, m]))) if np.isfinite(out[:, m]).any() else float("nan"))
    return res


def block_expectation(x32, F, form):
    """(expected, widening, truth = the accurate values, bands [3 + 6 F]) of one PE block"""
    bands = np.array([b for (_, b, _) in pe_columns(F)])
    return expected(x32, F, form), widening(x32, F, form), expected(x32, F, "accurate"), bands


# ---- the inputs of the fused sampling kernels, restated ---------------------------------------------------------------------------------------

def fit_ray_sample_depths(ident, p32, nds32, scene, reach=16):
    """the depths z_a of the raySampleInput points the DEVICE uses, read off the identity columns `ident` [A, n, 3] of
    adanerf_ray_features: the library's host code forms them with its own powf and torch.linspace's symmetric form (model_setup.cpp), a few
    ulp from O.ray_sample_depths in places, and the encoding is checked on the device's own x.  Per a: the one fp32 value within `reach` ulp
    of the oracle's under which fp32(fp32((p + nds z) / d1) d1) has the bits of every row; asserts that there is exactly one."""
    p32, nds32 = np.asarray(p32, np.float32), np.asarray(nds32, np.float32)
    d1 = np.float32(scene.depth_range[1])
    out = []
    for a, z0 in enumerate(O.ray_sample_depths(scene)):
        cand = (np.float32(z0).view(np.int32) + np.arange(-reach, reach + 1, dtype=np.int32)).view(np.float32)
        fits = []
        for z in cand:
            q = (p32 + (nds32 * z).astype(np.float32)).astype(np.float32)
            if np.array_equal(((q / d1).astype(np.float32) * d1).astype(np.float32), ident[a]):
                fits.append(z)
        assert len(fits) == 1, "raySampleInput point %d: %d depths within %d ulp of the oracle's reproduce the identity columns" % (a, len(fits), reach)
        out.append(fits[0])
    return np.array(out, np.float32)


def ray_sample_points(p32, nds32, scene, zs=None):
    """raySampleInput: (x [A, n, 3] = fp32((p + nds z_a) / d1), d1): what layer0_ray_samples encodes; its identity slots are fp32(x d1)
    (O.oracle_features).  zs: the depths z_a (default: the oracle's)"""
    zs = O.ray_sample_depths(scene) if zs is None else np.asarray(zs, np.float32)
    d1 = np.float32(scene.depth_range[1])
    p32, nds32 = np.asarray(p32, np.float32), np.asarray(nds32, np.float32)
    pts = (p32[None, :, :] + (nds32[None, :, :] * zs[:, None, None]).astype(np.float32)).astype(np.float32)
    return (pts / d1).astype(np.float32), d1


def sampling_expectation(u32, p32, nds32, scene, form, zs=None):
    """-> (s, E, truth [n, n_in0], bands [n_in0]) for the sampling network's whole input row, from the device's own unit direction u, sphere
    point p and ray direction nds (the raySampleInput blocks need the last, and the depths zs: ray_sample_points)"""
    fp, fd = scene.pos_enc[0]
    parts = [block_expectation(u32, fd, form), block_expectation(p32, fp, form)]
    if scene.ray_sample_input:
        xs, d1 = ray_sample_points(p32, nds32, scene, zs)
        for x in xs:
            s, E, t, b = block_expectation(x, fp, form)
            ident = (x * d1).astype(np.float32).astype(np.float64)
            s[:, :3], t[:, :3] = ident, ident
            parts.append((s, E, t, b))
    return tuple(np.concatenate([q[i] for q in parts], axis=-1) for i in range(4))


def shading_expectation(x32, d32, scene, form):
    """the same for the shading network's row [PE(x) | PE(d)]"""
    fp, fd = scene.pos_enc[1]
    parts = [block_expectation(x32, fp, form), block_expectation(d32, fd, form)]
    return tuple(np.concatenate([q[i] for q in parts], axis=-1) for i in range(4))


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------

STRADDLE_X = 195.3125      # 2^9 x 195.3125 = 1e5 exactly: pe_eval's wave-uniform range test flips inside the frame


def near_radius(F):
    """a view-cell radius under which every argument of an F-band encoding of a sphere point stays below 200 revolutions (and below 1e5
    radians); at most the base scene's 0.5"""
    return min(0.5, 200.0 * 2.0 * math.pi / 2.0 ** (F - 1))


def _cell(radius):
    s = 2.0 * radius / math.sqrt(3.0)
    return (s, s, s)


def scene_of(base, name, pe0=None, pe1=None, **kw):
    """dataclasses.replace of the base scene: (scene, [camera rotation], pose).  The camera sits at the view cell's centre, so the sphere
    point of a ray is centre + radius x direction.
      near      centre 0, radius near_radius(bands): every |a| < 256 revolutions and < 1e5;
      far       centre 0, radius 3.4, looking along +x, along +y and 10 degrees off +z (straight up the camera basis is undefined): the top
                band of p_x (p_y, p_z) passes 256 revolutions inside a cone of 22 degrees around the axis; the shading network sees the
                positions themselves (normalisation "None");
      straddle  centre (195.3125, 0, 0), radius 1, looking along +y: 2^9 p_x crosses 1e5 from one image column to the next."""
    pe = (tuple(pe0 or base.pos_enc[0]), tuple(pe1 or base.pos_enc[1]))
    if name == "near":
        sc = dataclasses.replace(base, view_cell_center=(0.0, 0.0, 0.0), view_cell_size=_cell(near_radius(max(pe[0][0], 1))), pos_enc=pe, **kw)
        rots = [O.camera_rotation(100.0, 0.0)]
    elif name == "far":
        sc = dataclasses.replace(base, view_cell_center=(0.0, 0.0, 0.0), view_cell_size=_cell(3.4), pos_enc=pe, normalization="None", **kw)
        rots = [O.camera_rotation(0.0, 0.0), O.camera_rotation(90.0, 0.0), O.camera_rotation(0.0, 80.0)]
    else:
        assert name == "straddle", name
        sc = dataclasses.replace(base, view_cell_center=(STRADDLE_X, 0.0, 0.0), view_cell_size=_cell(1.0), pos_enc=pe, normalization="None", **kw)
        rots = [O.camera_rotation(90.0, 0.0)]
    return sc, rots, np.array(sc.view_cell_center, np.float32)


def mixed(flag, block):
    """number of blocks of `block` consecutive rows that hold both kinds"""
    flag = np.asarray(flag, bool)
    n = -(-flag.size // block) * block
    a, b = np.zeros(n, bool), np.zeros(n, bool)
    a[:flag.size], b[:flag.size] = flag, ~flag
    return int((a.reshape(-1, block).any(axis=1) & b.reshape(-1, block).any(axis=1)).sum())


def conditions(name, xs, F):
    """What a scene has to put in front of the kernels, on the device's own x (xs: one [n, 3] per camera rotation) under an F-band encoding:
      near      every |a| below 256 revolutions and below 1e5;
      far       for each of the three components a camera rotation under which at least 25 % of its top-band arguments lie beyond 256
                revolutions;
      straddle  rows with an argument >= 1e5 and rows without, both kinds inside at least one 64-row wave and one 128-row tile.
    Asserts, and returns what is logged: the share of top-band arguments beyond 256 revolutions per component (the largest over the
    rotations), the largest |a| and, for straddle, the mixed 64-row waves and 128-row tiles."""
    rev = [revolutions(x, F) for x in xs]
    amax = max(float(np.abs(arguments(x, F)).max()) for x in xs)
    share = np.max([(r[:, F - 1, :] > REV_LIMIT).mean(axis=0) for r in rev], axis=0)
    info = dict(scene=name, bands=F, max_abs_a=amax, max_rev=float(max(r.max() for r in rev)), share_beyond_256=[float(v) for v in share])
    assert all(np.isfinite(x).all() for x in xs), name
    if name == "near":
        assert info["max_rev"] < REV_LIMIT and amax < SMALL_LIMIT, info
    elif name == "far":
        assert (share >= 0.25).all(), info
    else:
        big = np.abs(arguments(xs[0], F)).reshape(len(xs[0]), -1).max(axis=1) >= SMALL_LIMIT
        info.update(rows_beyond_1e5=int(big.sum()), mixed_waves=mixed(big, 64), mixed_tiles=mixed(big, 128))
        assert info["mixed_waves"] >= 1 and info["mixed_tiles"] >= 1 and 0 < big.sum() < big.size, info
    return info


# ---- the frame the CPU test runs on, and the GPU test's host-side twin --------------------------------------------------------------------------

def frame_inputs(scene, pose, rot, w=W, h=H):
    """(u, p, nds, features) of a w x h frame as the oracle computes them (fp32)"""
    nds, p = O.world_rays(O.generate_ray_directions(w, h, scene.fov), pose, rot, scene)
    nrm = np.sqrt(np.sum(nds * nds, axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    return (nds / nrm).astype(np.float32), p, nds, O.oracle_features(nds, p, scene)


def shade_keys(n_rays, n=N_SHADE, seed=5):
    """n distinct (ray << 7 | bin) keys in random order, bins 0 and 127 among them"""
    rng = np.random.default_rng(seed)
    key = np.unique((rng.integers(0, n_rays, 2 * n).astype(np.uint32) << 7) | rng.integers(0, 128, 2 * n).astype(np.uint32))
    key = key[rng.permutation(key.size)][:n]
    key[0], key[1] = key[0] & ~np.uint32(127), key[1] | np.uint32(127)
    assert np.unique(key).size == n
    return key
