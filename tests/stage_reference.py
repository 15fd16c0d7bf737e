"""fp64 restatements of the kernels around the two networks -- adaptive and classic compositing, the inverse-CDF sampler, the fine
sampler of the coarse/fine mode, the RGBA8 contract -- and the comparators the stage-kernel tests use.  Same role as mlp_reference.py:
plain numpy, float64 throughout, inputs taken as the fp32 values the kernel is given.  Written from this repository's kernels
(k_composite.hip.hpp, k_donerf.hip.hpp, k_coarse_fine.hip.hpp) and oracle.

Compositing is compared per ray in units of the forward error of an fp32 chain of that length:

    |K - ref64| <= C[kind] * 2^-24 * (n_samples + C0) * scale,      scale = sum_k |w_k| (fp64) + floor

w_k = alpha_k T_k.  Under mult weights the multiplier scales the weight but not the transmittance, which is what carries the rounding
of 1 - alpha_k to the later samples: the sum stays over alpha_k T_k and is multiplied by max(1, max_k |multiplier|) of the ray.

The floor is 2^-100 for the adaptive form: weights under the smallest normal fp32 number (2^-126; transmittances that ran into the
1e-10 floor several times over) may be flushed, n of them lose n 2^-126 <= 2^-24 n 2^-100.  The classic form forms alpha = 1 - exp(-x)
by a subtraction from 1: its absolute error is an ulp of 1 however small alpha is, so the chain also carries 2^-24 sum_k T_k, which
sum |w_k| does not see on a ray of small densities; there the floor is 2^-100 + mean_k |T_k|.  A component whose fp64 reference is
not finite must be non-finite in the kernel's output; no finite ray is excluded.

The depth and accumulation maps (acc = sum_k w_k, depth = sum_k w_k z_k, w_k the weight the colour is formed with: under mult weights
it carries the multiplier) are compared in the same units: acc against `scale`, depth against scale max_k |z_k| over the ray's active
samples (each term adds one rounding of w z), both with C_AUX[kind] in place of C[kind] and signed (multipliers in [-0.5, 1.8] make acc
negative on some rays).  z_k = ztab[key_k & 127], the table from adanerf_host_depth_table -- nothing a kernel wrote.  The non-finite rule is
the same.  C_AUX[kind] is twice the worst case of the fp32 emulations below against fp64 on the tests' own rows (MEASURED_AUX): the margin
the samplers and the colour constants have, for the association differences of a DPP scan; what the device measures does not widen it.

The samplers are compared by forward residual: the inverse CDF is ill-conditioned in empty bins, the CDF is not.  Every returned depth
is mapped back in fp64 and the fp64 CDF there must equal the sample's u.  The bound is twice the largest residual of the fp32 numpy
oracle on the same rows (sampler_bound); no sample is excluded.

Faults (``fault=``) of the fp32 emulations are the kernel bugs tests/test_stage_reference_cpu.py shows the comparators refuse."""
import numpy as np

F32 = np.float32
EPS = 2.0 ** -24
FLOOR = 2.0 ** -100
C0 = 8
E10 = float(F32(1e-10))
E5 = float(F32(1e-5))
MULT = {"": 0, "none": 0, "alpha": 1, "weights": 2, 0: 0, 1: 1, 2: 2}

# One constant per kernel family, in the units above: exactly twice the larger of the two measured worst cases -- `oracle`: the fp32
# numpy oracle against fp64 on the tests' inputs (recomputed and compared with this table by test_stage_reference_cpu.py); `device`: the
# kernel on an MI355X (the largest worst_units of its stage_kernel lines).  profiles/stage_kernels_measured.log has one line per kernel
# and case from both sides, and test_stage_reference_cpu.py compares this table with that log.  Figures are rounded up to 1e-4.
MEASURED = {
    "thread": dict(oracle=0.3915, device=0.3325),         # composite_kernel<256 / 128 / 64>: N = 1 alpha | N = 10 alpha
    "wave": dict(oracle=0.3858, device=0.4730),           # composite_wave_kernel: N = 64 alpha on both sides
    "classic_thread": dict(oracle=0.1109, device=0.1109), # composite_classic_kernel: n = 2, the same ray to the last bit
    "classic_wave": dict(oracle=0.0677, device=0.0465),   # composite_classic_wave_kernel: n = 65 | n = 1024
}
C = {k: 2 * max(v["oracle"], v["device"]) for k, v in MEASURED.items()}

# The maps: `emulation` is the larger of the depth and the acc worst case of composite32 / composite_classic32 (thread kinds: summed in
# sample order, wave kinds: per lane, then across the wave) against fp64 on the GPU tests' rows, all multiplier modes, the dense layout
# included; recomputed and compared with this table by test_stage_reference_cpu.py.  `device` is what an MI355X measured (the largest
# worst_units of its stage_kernel_aux lines in profiles/stage_kernels_measured.log); it is stated, and does not enter the bound.
MEASURED_AUX = {
    "thread": dict(emulation=0.3100, device=0.2792),          # composite_kernel<256>: depth, N = 1 alpha
    "wave": dict(emulation=0.4436, device=0.5682),            # composite_wave_kernel: acc, N = 64 alpha
    "classic_thread": dict(emulation=0.0629, device=0.0654),  # composite_classic_kernel: acc, n = 2
    "classic_wave": dict(emulation=0.0578, device=0.0487),    # composite_classic_wave_kernel: depth, n = 63
}
C_AUX = {k: 2 * v["emulation"] for k, v in MEASURED_AUX.items()}


def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def relu64(x):
    """torch.relu: 0 for x <= 0, NaN stays NaN"""
    x = np.asarray(x, np.float64)
    return np.where(x <= 0, 0.0, x)


def _excl_cumprod(f):
    return np.concatenate([np.ones_like(f[:, :1]), np.cumprod(f, 1)[:, :-1]], 1)


def gather(off, cnt):
    """[R, n] sample indices and the active mask of a (offset, count) layout; inactive slots index sample 0"""
    n = int(cnt.max()) if cnt.size else 0
    act = np.arange(n)[None, :] < cnt[:, None]
    return np.where(act, off[:, None].astype(np.int64) + np.arange(n)[None, :], 0), act


# ---- a. compositing ---------------------------------------------------------------------------------------------------------------------

def composite64(raw, sample_w, off, cnt, mult, z=None):
    """The adaptive form (k_composite.hip.hpp composite_step): sigmoid on the four channels, alpha *= oracle value (mult alpha),
    w = alpha prod_{j<k} (1 - alpha_j + 1e-10), w *= oracle value (mult weights).  -> rgb [R,3], depth, acc, scale [R]"""
    m = MULT[mult]
    idx, act = gather(off, cnt)
    with np.errstate(all="ignore"):
        s = sigmoid64(raw[idx])
        wv = np.where(act, sample_w[idx].astype(np.float64), 0.0)
        al = np.where(act, s[..., 3], 0.0)
        if m == 1:
            al = al * wv
        T = _excl_cumprod(np.where(act, 1.0 - al + E10, 1.0))
        w = al * T
        # mult weights scales the weight, not the transmittance that carries the rounding of 1 - alpha to the later samples: the
        # scale is taken over alpha_k T_k, times the largest multiplier of the ray where that exceeds 1
        scale = np.sum(np.abs(np.where(act, w, 0.0)), 1) + FLOOR
        if m == 2:
            w = w * wv
            scale = scale * np.maximum(1.0, np.max(np.abs(wv), 1, initial=0.0))
        w = np.where(act, w, 0.0)
        rgb = np.sum(w[..., None] * np.where(act[..., None], s[..., :3], 0.0), 1)
        acc = np.sum(w, 1)
        depth = np.sum(w * np.where(act, np.asarray(z, np.float64)[idx], 0.0), 1) if z is not None else np.zeros_like(acc)
    return rgb.reshape(-1, 3), depth, acc, scale


def composite_classic64(raw, z, rays_d):
    """The classic form (k_donerf.hip.hpp): alpha = 1 - exp(-relu(sigma) (z[k+1] - z[k]) |d|), last interval 1e10, the 1e-10
    transmittance floor.  raw [R,n,4], z [R,n], rays_d [R,3] -> rgb, depth, acc, scale"""
    raw, z, d = np.asarray(raw, np.float64), np.asarray(z, np.float64), np.asarray(rays_d, np.float64)
    with np.errstate(all="ignore"):
        dn = np.sqrt(np.sum(d * d, -1, keepdims=True))
        dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((z.shape[0], 1), 1e10)], 1) * dn
        al = 1.0 - np.exp(-relu64(raw[..., 3]) * dist)
        T = _excl_cumprod(1.0 - al + E10)
        w = al * T
        rgb = np.sum(w[..., None] * sigmoid64(raw[..., :3]), 1)
        scale = np.sum(np.abs(w), 1) + np.mean(np.abs(T), 1) + FLOOR
        return rgb, np.sum(w * z, 1), np.sum(w, 1), scale


def composite_units(K, ref, scale, n_samples):
    """|K - ref| in units of 2^-24 (n + C0) scale, and the verdict of the non-finite rule; K, ref [R] or [R,c]"""
    K, ref = np.asarray(K, np.float64), np.asarray(ref, np.float64)
    K2, ref2 = K.reshape(K.shape[0], -1), ref.reshape(ref.shape[0], -1)
    fin = np.isfinite(ref2)
    nonfinite_ok = bool((~np.isfinite(K2[~fin])).all())
    unit = (EPS * (np.asarray(n_samples, np.float64) + C0) * scale).reshape(-1, 1)
    with np.errstate(all="ignore"):
        u = np.where(fin & (K2 != ref2), np.abs(K2 - ref2) / unit, 0.0)      # an empty ray's depth has unit 0: only exactly 0 passes
    u = np.where(fin & ~np.isfinite(K2), np.inf, u)          # a finite reference and a non-finite result: never inside a bound
    return u, nonfinite_ok


def check_composite(K, ref, scale, n_samples, kind, log=None, bound=None):
    """The comparator of every compositing kernel; returns the worst case in the bound's units (recorded through `log` first)"""
    u, ok = composite_units(K, ref, scale, n_samples)
    worst = float(u.max()) if u.size else 0.0
    b = C[kind] if bound is None else bound
    if log:
        log(dict(kind=kind, worst_units=worst, bound=b, rays=int(u.shape[0]), non_finite_rule=ok))
    assert ok, "%s: a component whose fp64 reference is not finite came out finite" % kind
    assert worst <= b, "%s: worst ray %d is %.3g units of 2^-24 (n + %d) scale off fp64 (bound %.3g)" % (
        kind, int(np.argmax(u.max(1))), worst, C0, b)
    return worst


def ray_zmax(z, off, cnt):
    """max_k |z_k| over the active samples of each ray of an (offset, count) layout (0 for an empty ray); z [S]"""
    idx, act = gather(off, cnt)
    return np.max(np.where(act, np.abs(np.asarray(z, np.float64)[idx]), 0.0), 1, initial=0.0)


def check_aux(depth, acc, ref_depth, ref_acc, scale, zmax, n_samples, kind, log=None):
    """The comparator of the two maps (either may be None: not requested); returns the worst cases (depth, acc) in the bound's units"""
    worst = {}
    for name, K, ref, sc in (("depth", depth, ref_depth, scale * zmax), ("acc", acc, ref_acc, scale)):
        if K is None:
            continue
        u, ok = composite_units(K, ref, sc, n_samples)
        worst[name] = float(u.max()) if u.size else 0.0
        if log:
            log(dict(kind=kind, map=name, worst_units=worst[name], bound=C_AUX[kind], rays=int(u.shape[0]), non_finite_rule=ok))
        assert ok, "%s %s: a ray whose fp64 reference is not finite came out finite" % (kind, name)
        assert worst[name] <= C_AUX[kind], "%s %s: worst ray %d is %.3g units of 2^-24 (n + %d) scale off fp64 (bound %.3g)" % (
            kind, name, int(np.argmax(u.max(1))), worst[name], C0, C_AUX[kind])
    return worst.get("depth", 0.0), worst.get("acc", 0.0)


def _seq_sum(x):
    return np.cumsum(x, 1, dtype=F32)[:, -1] if x.shape[1] else np.zeros(x.shape[0], F32)


def _wave_sum(x):
    """each lane adds its values (sample lane, lane + 64, ...) in order, then the wave sums the 64 lanes"""
    R, n = x.shape
    laps = max((n + 63) // 64, 1)
    p = np.zeros((R, laps * 64), F32)
    p[:, :n] = x
    return np.sum(np.cumsum(p.reshape(R, laps, 64), 1, dtype=F32)[:, -1], 1, dtype=F32)


def composite32(raw, sample_w, off, cnt, mult, fault=None, ztab=None, key=None, order="wave"):
    """fp32 emulation of the wave kernel's arithmetic (two 64-sample halves, the second scaled by the first's total) with its faults:
    inclusive (product includes the sample's own factor), no_half_total, mult2_on_alpha.  With a depth table `ztab` [128] (and `key` [S];
    None: bin = sample index & 127) -> (rgb, depth, acc) with the maps as the kernels form them: products rounded, then summed per lane
    and across the wave (order = "wave") or in sample order with a sequential transmittance (order = "seq": composite_kernel).  Faults of
    the maps: z_by_index (the table looked up by index & 127 although a key is given), aux_without_mult (mult weights: the map's weight
    lacks the multiplier), aux_second_half_unmasked (slots >= count of the second half contribute what lies there)"""
    if ztab is None:
        return _composite32(raw, sample_w, off, cnt, mult, fault, order)[0]
    idx, act = gather(off, cnt)
    S = raw.shape[0]
    rgb, q, w_plain = _composite32(raw, sample_w, off, cnt, mult, fault, order)
    if fault == "aux_second_half_unmasked":
        k = np.arange(act.shape[1])[None, :]
        act = act | (k >= 64)
        idx = np.minimum(off[:, None].astype(np.int64) + k, S - 1)
        _, q, w_plain = _composite32(raw, sample_w, off, cnt, mult, fault, order, idx, act)
    if fault == "aux_without_mult":
        q = w_plain
    bins = (idx if (key is None or fault == "z_by_index") else np.asarray(key).astype(np.int64)[idx]) & 127
    with np.errstate(all="ignore"):
        z = np.where(act, np.asarray(ztab, F32)[bins], F32(0))
        q = np.where(act, q, F32(0))
        add = _seq_sum if order == "seq" else _wave_sum
        return rgb, add((q * z).astype(F32)), add(q)


def _composite32(raw, sample_w, off, cnt, mult, fault, order, idx=None, act=None):
    """-> rgb, the samples' weights [R,n] (with the multiplier of mult weights), and without it"""
    m = MULT[mult]
    if idx is None:
        idx, act = gather(off, cnt)
    chunk = 64 if order == "wave" else max(act.shape[1], 1)
    with np.errstate(all="ignore"):
        s = (F32(1) / (F32(1) + np.exp(-raw[idx].astype(F32), dtype=F32))).astype(F32)
        wv = np.where(act, sample_w[idx].astype(F32), F32(0))
        al = np.where(act, s[..., 3], F32(0))
        if m == 1 or (m == 2 and fault == "mult2_on_alpha"):
            al = (al * wv).astype(F32)
        f = np.where(act, (F32(1) - al) + F32(1e-10), F32(1)).astype(F32)
        T = np.ones_like(f)
        for h in range(0, f.shape[1], chunk):
            p = np.cumprod(f[:, h:h + chunk], 1, dtype=F32)
            e = p if fault == "inclusive" else np.concatenate([np.ones_like(p[:, :1]), p[:, :-1]], 1)
            carry = np.ones_like(p[:, :1]) if (h == 0 or fault == "no_half_total") else np.prod(f[:, :h], 1, dtype=F32)[:, None]
            T[:, h:h + chunk] = carry * e
        w = w_plain = (al * T).astype(F32)
        if m == 2 and fault != "mult2_on_alpha":
            w = (w * wv).astype(F32)
        return np.sum(w[..., None] * np.where(act[..., None], s[..., :3], F32(0)), 1, dtype=F32).reshape(-1, 3), w, w_plain


def composite_classic32(raw, z, rays_d, fault=None, aux=False, order="wave"):
    """fp32 emulation of the classic wave kernel (64-sample laps, transmittance carried) with its faults: no_lap_carry, last_zero, no_relu.
    aux -> (rgb, depth, acc), the maps summed per lane over the laps and then across the wave (order = "wave") or in sample order
    ("seq": composite_classic_kernel); their fault: classic_depth_next_z (z[k+1] in place of z[k], 0 after the last)"""
    raw, z, d = raw.astype(F32), z.astype(F32), rays_d.astype(F32)
    with np.errstate(all="ignore"):
        dn = np.sqrt(np.sum(d * d, -1, keepdims=True, dtype=F32))
        last = F32(0) if fault == "last_zero" else F32(1e10)
        dist = (np.concatenate([z[:, 1:] - z[:, :-1], np.full((z.shape[0], 1), last, F32)], 1) * dn).astype(F32)
        sg = raw[..., 3] if fault == "no_relu" else np.where(raw[..., 3] <= 0, F32(0), raw[..., 3])
        al = (F32(1) - np.exp(-sg * dist, dtype=F32)).astype(F32)
        f = ((F32(1) - al) + F32(1e-10)).astype(F32)
        T = np.ones_like(f)
        for h in range(0, f.shape[1], 64):
            p = np.cumprod(f[:, h:h + 64], 1, dtype=F32)
            e = np.concatenate([np.ones_like(p[:, :1]), p[:, :-1]], 1)
            carry = np.ones_like(p[:, :1]) if (h == 0 or fault == "no_lap_carry") else np.prod(f[:, :h], 1, dtype=F32)[:, None]
            T[:, h:h + 64] = carry * e
        w = (al * T).astype(F32)
        s = (F32(1) / (F32(1) + np.exp(-raw[..., :3], dtype=F32))).astype(F32)
        rgb = np.sum(w[..., None] * s, 1, dtype=F32)
        if not aux:
            return rgb
        zz = np.concatenate([z[:, 1:], np.zeros_like(z[:, :1])], 1) if fault == "classic_depth_next_z" else z
        add = _seq_sum if order == "seq" else _wave_sum
        return rgb, add((w * zz).astype(F32)), add(w)


# ---- c. RGBA8 -------------------------------------------------------------------------------------------------------------------------

def rgba8_of(rgb32, fault=None):
    """The viewer contract as the kernels write it: fmaxf(v, 0) (NaN -> 0), fminf(., 1), * 255 in fp32, truncate; A = 255"""
    v = np.asarray(rgb32, F32).reshape(-1, 3)
    v = np.where(np.isnan(v), F32(0), v)
    v = (np.minimum(np.maximum(v, F32(0)), F32(1)) * F32(255.0)).astype(F32)
    if fault == "round":
        v = np.floor(v + F32(0.5))
    out = np.full((v.shape[0], 4), 255, np.uint8)
    out[:, :3] = v.astype(np.uint8)
    return out


# ---- b. the inverse-CDF sampler ---------------------------------------------------------------------------------------------------------

TRANSFORMS = {"BCEWithLogitsLoss": "sigmoid", "CrossEntropyLoss": "softmax", "CrossEntropyLossWeighted": "softmax"}


def pdf_cdf64(orc, losses0):
    """fp64 CDF over the 129 bin edges of transform(oracle row) + 1e-5"""
    x = np.asarray(orc, np.float64)
    t = TRANSFORMS.get(losses0, "none")
    with np.errstate(all="ignore"):
        if t == "sigmoid":
            x = sigmoid64(x)
        elif t == "softmax":
            e = np.exp(x - np.max(x, -1, keepdims=True))
            x = e / np.sum(e, -1, keepdims=True)
        w = x + E5
        pdf = w / np.sum(w, -1, keepdims=True)
        return np.concatenate([np.zeros_like(pdf[:, :1]), np.cumsum(pdf, -1)], -1)


def from_world64(z, depth_range, log):
    d0, d1 = float(F32(depth_range[0])), float(F32(depth_range[1]))
    z = np.asarray(z, np.float64)
    with np.errstate(all="ignore"):
        return np.log(z - d0 + 1.0) / np.log(d1 - d0 + 1.0) if log else (z - d0) / (d1 - d0)


def pdf_residual(z_world, orc, n, losses0, depth_range, log):
    """CDF64(warped depth of every sample) - u, [R,n]; and the warped depths"""
    cdf = pdf_cdf64(orc, losses0)
    B = cdf.shape[1] - 1
    t = from_world64(np.asarray(z_world).reshape(-1, n), depth_range, log)
    with np.errstate(all="ignore"):
        b = np.clip(np.floor(np.nan_to_num(t) * B), 0, B - 1).astype(np.int64)
        c0, c1 = np.take_along_axis(cdf, b, 1), np.take_along_axis(cdf, b + 1, 1)
        val = c0 + (t * B - b) * (c1 - c0)
    u = (np.arange(n, dtype=np.float64) + 1.0) / (n + 1.0)
    return val - u[None, :], t


def sampler_bound(oracle_residual):
    """twice the fp32 numpy oracle's largest residual on the same rows"""
    return 2.0 * float(np.max(np.abs(oracle_residual)))


def check_pdf(z_world, key, w, off, cnt, total, orc, n, losses0, depth_range, log_depth, bound, finite_rows=None, log=None):
    """Every sample of every (finite) row: forward residual, ascending depths, the key's bin, zero weights; exact bookkeeping everywhere"""
    R = orc.shape[0]
    assert int(total) == R * n and np.array_equal(cnt, np.full(R, n, np.int32)) and np.array_equal(off, np.arange(R, dtype=np.int64) * n)
    key = np.asarray(key).reshape(R, n)
    assert np.array_equal(key >> 7, np.repeat(np.arange(R, dtype=np.uint32)[:, None], n, 1)), "key: ray field"
    assert (np.asarray(w).view(np.uint32) == 0).all(), "sample_w != +0"
    fin = np.ones(R, bool) if finite_rows is None else np.asarray(finite_rows, bool)
    res, t = pdf_residual(z_world, orc, n, losses0, depth_range, log_depth)
    res, t = res[fin], t[fin]
    worst = float(np.abs(res).max()) if res.size else 0.0
    if log:
        log(dict(n=n, worst_residual=worst, bound=bound, rows=int(fin.sum())))
    assert np.isfinite(res).all() and worst <= bound, "largest residual %.3g > %.3g (n = %d)" % (worst, bound, n)
    zz = np.asarray(z_world).reshape(R, n)[fin]
    assert (np.diff(zz, axis=1) >= 0).all(), "depths do not ascend"
    # the key's bin: the depth lies in it (closed, to the fp32 rounding of the depth transform) and its CDF interval holds u to the residual
    cdf = pdf_cdf64(orc, losses0)[fin]
    kb = (key[fin] & 127).astype(np.int64)
    B = cdf.shape[1] - 1
    u = ((np.arange(n, dtype=np.float64) + 1.0) / (n + 1.0))[None, :]
    inside = (t * B >= kb - 1e-4) & (t * B <= kb + 1 + 1e-4)
    holds = (u >= np.take_along_axis(cdf, kb, 1) - bound) & (u <= np.take_along_axis(cdf, kb + 1, 1) + bound)
    assert inside.all() and holds.all(), "key bin: %d depths outside their bin, %d bins whose CDF interval misses u" % ((~inside).sum(), (~holds).sum())
    return worst


def pdf32(orc, n, losses0, fault=None):
    """fp32 emulation of pdf_sample_kernel (two 64-bin halves) -> warped depths [R,n]; faults: no_eps, u_k_over_n, no_lower_total"""
    x = np.asarray(orc, F32)
    t = TRANSFORMS.get(losses0, "none")
    with np.errstate(all="ignore"):
        if t == "sigmoid":
            x = (F32(1) / (F32(1) + np.exp(-x, dtype=F32))).astype(F32)
        elif t == "softmax":
            e = np.exp(x - np.max(x, -1, keepdims=True), dtype=F32)
            x = (e / np.sum(e, -1, keepdims=True, dtype=F32)).astype(F32)
        w = x if fault == "no_eps" else (x + F32(1e-5)).astype(F32)
        p = (w / np.sum(w, -1, keepdims=True, dtype=F32)).astype(F32)
        cA = np.cumsum(p[:, :64], 1, dtype=F32)
        cB = np.cumsum(p[:, 64:], 1, dtype=F32)
        if fault != "no_lower_total":
            cB = (cA[:, 63:64] + cB).astype(F32)
        cdf = np.concatenate([np.zeros_like(cA[:, :1]), cA, cB], 1)
        k = np.arange(n, dtype=F32)
        u = (k / F32(n)) if fault == "u_k_over_n" else ((k + F32(1)) / F32(n + 1))
        u = u.astype(F32)
        out = np.empty((x.shape[0], n), F32)
        for r in range(x.shape[0]):
            lo = np.searchsorted(cdf[r], u, side="right")
            below, above = np.maximum(lo - 1, 0), np.minimum(lo, 128)
            c0, c1 = cdf[r][below], cdf[r][above]
            den = (c1 - c0).astype(F32)
            den = np.where(den < F32(1e-5), F32(1), den)
            tt = ((u - c0) / den).astype(F32)
            b0, b1 = below.astype(F32) * F32(1 / 128), above.astype(F32) * F32(1 / 128)
            out[r] = (b0 + tt * (b1 - b0)).astype(F32)
        return out


# ---- b. the fine sampler ------------------------------------------------------------------------------------------------------------------

def fine_cdf64(raw_coarse, zc, rays_d):
    """fp64 CDF over the nc - 1 interval mid-points from fp64 classic weights[1 : nc-1] + 1e-5; -> (cdf [R, nc-1], mids [nc-1])"""
    raw = np.asarray(raw_coarse, np.float64)
    zc = np.asarray(zc, np.float64)
    d = np.asarray(rays_d, np.float64)
    R, nc = raw.shape[0], zc.shape[0]
    with np.errstate(all="ignore"):
        dn = np.sqrt(np.sum(d * d, -1, keepdims=True))
        dist = np.concatenate([np.repeat((zc[1:] - zc[:-1])[None], R, 0), np.full((R, 1), 1e10)], 1) * dn
        al = 1.0 - np.exp(-relu64(raw[..., 3]) * dist)
        wts = al * _excl_cumprod(1.0 - al + E10)
        w = wts[:, 1:-1] + E5
        pdf = w / np.sum(w, -1, keepdims=True)
        cdf = np.concatenate([np.zeros((R, 1)), np.cumsum(pdf, -1)], -1)
    return cdf, 0.5 * (zc[1:] + zc[:-1])


def split_fine_rows(rows, zc32, nf):
    """Removes one copy of each coarse depth (bit for bit) from every row -> the nf new depths per row, in the row's order"""
    rows = np.asarray(rows, F32)
    out = np.empty((rows.shape[0], nf), F32)
    for r in range(rows.shape[0]):
        row = rows[r]
        keep = np.ones(row.shape[0], bool)
        bits = row.view(np.uint32)
        j = 0
        for v in zc32.view(np.uint32):                # both ascend: one forward walk
            while j < row.shape[0] and (bits[j] != v or not keep[j]):
                j += 1
            assert j < row.shape[0], "row %d: coarse depth %r is not in the output" % (r, zc32.view(np.uint32).tolist().index(int(v)))
            keep[j] = False
            j += 1
        assert int(keep.sum()) == nf, "row %d: %d values left after removing the coarse depths, not %d" % (r, int(keep.sum()), nf)
        out[r] = row[keep]
    return out


def fine_residual(z_new, raw_coarse, zc32, rays_d, nf):
    cdf, mids = fine_cdf64(raw_coarse, zc32, rays_d)
    z = np.asarray(z_new, np.float64)
    nb = mids.shape[0]
    b = np.clip(np.searchsorted(mids, np.nan_to_num(z), side="right") - 1, 0, nb - 2)
    with np.errstate(all="ignore"):
        frac = np.clip((z - mids[b]) / (mids[b + 1] - mids[b]), 0.0, 1.0) if nb > 1 else np.zeros_like(z)
        c0, c1 = np.take_along_axis(cdf, b, 1), np.take_along_axis(cdf, np.minimum(b + 1, nb - 1), 1)
        val = c0 + frac * (c1 - c0)
    u = np.arange(nf, dtype=np.float64) / max(nf - 1, 1)
    return val - u[None, :]


def check_fine(rows, raw_coarse, zc32, rays_d, nf, bound, log=None):
    """rows [R, nc + nf] of finite rays: ascending; the nc coarse depths bit for bit; exactly nf others, each by forward residual"""
    rows = np.asarray(rows, F32)
    assert (np.diff(rows, axis=1) >= 0).all(), "merged depths do not ascend"
    new = split_fine_rows(rows, np.asarray(zc32, F32), nf)
    assert (np.diff(new, axis=1) >= 0).all(), "new depths decrease in u order"
    res = fine_residual(new, raw_coarse, zc32, rays_d, nf)
    worst = float(np.abs(res).max()) if res.size else 0.0
    if log:
        log(dict(nc=int(len(zc32)), nf=nf, worst_residual=worst, bound=bound, rows=int(rows.shape[0])))
    assert np.isfinite(res).all() and worst <= bound, "largest residual %.3g > %.3g (nc %d, nf %d)" % (worst, bound, len(zc32), nf)
    return worst


def fine32(raw_coarse, zc32, rays_d, nf, fault=None):
    """fp32 emulation of fine_sample_kernel -> merged rows [R, nc + nf]; faults: w0_in_pdf, drop_coarse, dup_coarse"""
    raw, zc, d = np.asarray(raw_coarse, F32), np.asarray(zc32, F32), np.asarray(rays_d, F32)
    R, nc = raw.shape[0], zc.shape[0]
    with np.errstate(all="ignore"):
        dn = np.sqrt(np.sum(d * d, -1, keepdims=True, dtype=F32))
        dist = (np.concatenate([np.repeat((zc[1:] - zc[:-1])[None], R, 0), np.full((R, 1), 1e10, F32)], 1) * dn).astype(F32)
        al = (F32(1) - np.exp(-np.where(raw[..., 3] <= 0, F32(0), raw[..., 3]) * dist, dtype=F32)).astype(F32)
        T = _excl_cumprod(((F32(1) - al) + F32(1e-10)).astype(np.float64)).astype(F32)
        wts = (al * T).astype(F32)
        w = wts[:, 1:-1]
        if fault == "w0_in_pdf":        # the pdf built over weights[0 : nc-2]: one interval early
            w = wts[:, 0:-2]
        w = (w + F32(1e-5)).astype(F32)
        pdf = (w / np.sum(w.astype(np.float64), -1, keepdims=True).astype(F32)).astype(F32)
        cdf = np.concatenate([np.zeros((R, 1), F32), np.cumsum(pdf.astype(np.float64), -1).astype(F32)], -1)
        mids = (F32(0.5) * (zc[1:] + zc[:-1])).astype(F32)
        u = np.linspace(0.0, 1.0, nf, dtype=F32) if nf > 1 else np.zeros(1, F32)
        out = np.empty((R, nc + nf), F32)
        for r in range(R):
            lo = np.searchsorted(cdf[r], u, side="right")
            below, above = np.maximum(lo - 1, 0), np.minimum(lo, nc - 2)
            c0, c1 = cdf[r][below], cdf[r][above]
            den = (c1 - c0).astype(F32)
            den = np.where(den < F32(1e-5), F32(1), den)
            zf = (mids[below] + ((u - c0) / den).astype(F32) * (mids[above] - mids[below])).astype(F32)
            co = zc
            if fault == "drop_coarse":
                co = np.concatenate([zc[:nc // 2], zc[nc // 2 + 1:], zf[-1:]])      # one coarse depth lost, the row keeps its length
            elif fault == "dup_coarse":
                co, zf = np.concatenate([zc, zc[nc // 2:nc // 2 + 1]]), zf[:-1]     # one written twice, the last new depth pushed out
            out[r] = np.sort(np.concatenate([co, zf]))
        return out


# ---- inputs (seeded; the CPU and the GPU tests run the same ones) ------------------------------------------------------------------------

def _raw_rows(rng, shape):
    """raw network outputs: the spread of trained nets (|x| up to ~30), of untrained nets (N(0, 4)), saturated +-100"""
    x = rng.normal(0.0, 2.0, shape)
    kind = rng.random(shape[:-1] + (1,))
    x = np.where(kind < 0.35, rng.uniform(-30.0, 30.0, shape), x)
    x = np.where(rng.random(shape) < 0.04, np.where(rng.random(shape) < 0.5, 100.0, -100.0), x)
    return x.astype(F32)


NONFINITE = (np.nan, np.inf, -np.inf)


def composite_inputs(seed, N, n_rays=192, nonfinite=True):
    """A base set of distinct rays in the compactor's layout: counts ragged in 0..N (count 0 rays between non-empty ones, full rays),
    saturating runs, rows of identical samples, oracle weights in [-0.5, 1.8], and a few rays carrying NaN / +-inf (finite_rays = False)
    -> dict(raw [S,4], sw [S], off, cnt [R] int32, finite [R] bool, key [S] uint32: ray << 7 | bin, the bins of a ray ascending and
    distinct over 0..127 as the compactor produces them (drawn from a generator of their own: the other arrays are what they were))"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, N + 1, n_rays)
    cnt[:12] = [N, 0, N, 1 if N > 1 else N, 0, 0, N, max(N - 1, 0), min(64, N), min(65, N), min(63, N), N]
    cnt[12:24] = N
    cnt = cnt.astype(np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    S = int(cnt.sum())
    raw = _raw_rows(rng, (S, 4))
    sw = rng.uniform(-0.5, 1.8, S).astype(F32)
    sw = np.where(rng.random(S) < 0.5, rng.uniform(0.0, 1.0, S), sw).astype(F32)      # half of them what a trained net gives
    ray = np.repeat(np.arange(n_rays), cnt)
    pos = np.arange(S) - off[ray]
    sel = lambda r: ray == r
    raw[sel(12)] = raw[off[12]]                       # a row of identical samples
    sw[sel(12)] = sw[off[12]]
    raw[sel(13), 3] = -100.0                          # alpha exactly 0 all along
    raw[sel(14), 3] = 100.0                           # alpha exactly 1: T runs into the 1e-10 floor and underflows
    sw[sel(14)] = 1.0
    raw[sel(15) & (pos % 2 == 0), 3] = 100.0          # alternating 1 / 0
    raw[sel(15) & (pos % 2 == 1), 3] = -100.0
    raw[sel(16), 3] = -8.0                            # small alphas: T stays near 1 over the whole ray
    finite = np.ones(n_rays, bool)
    if nonfinite:
        for j, r in enumerate(range(24, min(36, n_rays))):      # NaN / inf in one channel of one sample, first / middle / last
            if cnt[r] == 0:
                continue
            k = off[r] + (0, cnt[r] // 2, cnt[r] - 1)[j % 3]
            raw[k, (j // 3) % 4] = NONFINITE[j % 3]
            finite[r] = False
        for r in (36, 37):
            if r < n_rays and cnt[r] > 0:
                sw[off[r] + cnt[r] // 2] = np.nan if r == 36 else np.inf
                finite[r] = False
    krng = np.random.default_rng(seed + 7000000)
    bins = np.concatenate([np.sort(krng.permutation(128)[:c]) for c in cnt] + [np.zeros(0, np.int64)])
    key = ((ray.astype(np.uint32) << np.uint32(7)) | bins.astype(np.uint32)).astype(np.uint32)
    return dict(raw=raw, sw=sw, off=off, cnt=cnt, finite=finite, key=key)


def permuted(L, B):
    """ray j of the long list is base ray (a j + c) mod B"""
    return (7919 * np.arange(L, dtype=np.int64) + 17) % B


def layout(c, ids, gap=None):
    """The base rays `ids`, in that order, as a fresh (offset, count) layout: the compactor's without `gap`, with gap[i] unused slots
    (NaN, key of all ones: nothing may read them) in front of ray i otherwise -> raw, sw, off, cnt, key"""
    cnt = c["cnt"][ids].astype(np.int64)
    g = np.zeros_like(cnt) if gap is None else np.asarray(gap, np.int64)
    start = np.cumsum(cnt + g) - cnt
    total = int(start[-1] + cnt[-1])
    intra = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    src = np.repeat(c["off"][ids].astype(np.int64), cnt) + intra
    dst = np.repeat(start, cnt) + intra
    raw = np.full((max(total, 1), 4), np.nan, np.float32)
    sw = np.full(max(total, 1), np.nan, np.float32)
    key = np.full(max(total, 1), 0xFFFFFFFF, np.uint32)
    raw[dst], sw[dst], key[dst] = c["raw"][src], c["sw"][src], c["key"][src]
    return raw, sw, start.astype(np.int32), cnt.astype(np.int32), key


def dense_layout(n_rays=1001):
    """test_composite_dense_mode's rows: the 128-sample rays of composite_inputs(1128, 128), permuted, in the compactor's layout"""
    c = composite_inputs(1128, 128)
    ids = np.flatnonzero(c["cnt"] == 128)
    raw, sw, off, cnt, key = layout(c, ids[permuted(n_rays, ids.size)])
    return dict(raw=raw, sw=sw, off=off, cnt=cnt, key=key)


def host_depth_table(lib, options_type, model_dir, num_samples, threshold):
    """The context's depth table [128] from the host library (adanerf_host_depth_table: compared with the oracle in test_host_cpu.py)"""
    import ctypes
    lib.adanerf_host_depth_table.argtypes = [ctypes.c_char_p, ctypes.POINTER(options_type), ctypes.c_void_p]
    o = options_type(width=8, height=8, batch_rays=0, device_id=0, precision=0, num_samples=num_samples, threshold=threshold, shard_rank=0,
                     shard_world=1, strip_rows=8)
    zt = np.zeros(128, F32)
    rc = lib.adanerf_host_depth_table(model_dir.encode(), ctypes.byref(o), zt.ctypes.data)
    assert rc == 0, lib.adanerf_last_error(None)
    return zt


def classic_inputs(seed, n, n_rays=96, nonfinite=True):
    """raw [R,n,4], z [R,n] ascending world depths (with equal consecutive depths), rays [R,8] with |d| from 0.1 to 30, finite [R]"""
    rng = np.random.default_rng(seed)
    raw = _raw_rows(rng, (n_rays, n, 4))
    raw[..., 3] = np.where(rng.random((n_rays, n)) < 0.5, rng.normal(0.0, 2.0, (n_rays, n)), rng.uniform(-5.0, 30.0, (n_rays, n)))
    z = np.sort(rng.uniform(0.5, 12.0, (n_rays, n)), 1).astype(F32)
    eq = rng.random((n_rays, n)) < 0.08
    for k in range(1, n):
        z[:, k] = np.where(eq[:, k], z[:, k - 1], z[:, k])      # zero intervals
    raw[0:4, :, 3] = [[-3.0], [0.0], [100.0], [1e-3]]            # all negative / all zero / opaque at once / thin all along
    raw[4, :, 3] = -1.0
    raw[4, -1, 3] = 1e30                                         # nothing until a huge density in the last sample
    raw[5, :, 3] = 0.05
    raw[5, -1, 3] = 3e38
    raw[6] = raw[6, 0]                                           # identical samples
    raw[7, :, 3] = 100.0                                         # T reaches the 1e-10 floor and underflows across the ray
    d = rng.normal(0.0, 1.0, (n_rays, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(0.1), np.log(30.0), (n_rays, 1)))
    rays = np.zeros((n_rays, 8), F32)
    rays[:, 0:3] = rng.normal(0.0, 1.0, (n_rays, 3))
    rays[:, 4:7] = d
    finite = np.ones(n_rays, bool)
    if nonfinite:
        for j, r in enumerate(range(8, min(20, n_rays))):
            raw[r, (0, n // 2, n - 1)[j % 3], (j // 3) % 4] = NONFINITE[j % 3]
            finite[r] = False
    return dict(raw=raw.astype(F32), z=z, rays=rays, finite=finite)


def pdf_rows(seed, losses0, n_rows=160, nonfinite=True):
    """Sampling-network rows [R,128] as the transform of `losses0` expects them (logits; non-negative values for no transform): peaky,
    near-empty (logits -30 with one to three peaks), all-equal, mass in bin 0 / in bin 127 / straddling bins 63 | 64; finite [R]"""
    rng = np.random.default_rng(seed)
    x = rng.normal(-2.0, 3.0, (n_rows, 128))
    for r in range(n_rows // 2):                                 # near-empty with one to three peaks
        x[r] = -30.0
        for _ in range(1 + r % 3):
            x[r, rng.integers(0, 128)] = rng.uniform(-1.0, 8.0)
    x[0] = -30.0
    x[0, 0] = 6.0                                                # mass in bin 0
    x[1] = -30.0
    x[1, 127] = 6.0                                              # mass in bin 127
    x[2] = -30.0
    x[2, 63:65] = [5.0, 5.5]                                     # straddling the two halves
    x[3] = 0.7                                                   # all equal
    x[4] = -30.0                                                 # empty: the 1e-5 alone
    x[5] = 30.0                                                  # saturated
    x[6, :] = -30.0
    x[6, 60:70] = np.linspace(-2.0, 7.0, 10)
    if TRANSFORMS.get(losses0, "none") == "none":
        with np.errstate(over="ignore"):
            x = 1.0 / (1.0 + np.exp(-x))                         # values a sampler without a transform sees: non-negative
    x = x.astype(F32)
    finite = np.ones(n_rows, bool)
    if nonfinite:
        for j, r in enumerate(range(8, 14)):
            x[r, (0, 64, 127)[j % 3]] = NONFINITE[j % 3] if j < 3 else np.nan
            finite[r] = False
    return x, finite


def fine_inputs(seed, nc, n_rays=128, nonfinite=True):
    """coarse network outputs [R,nc,4] and ray records [R,8]; finite [R]"""
    c = classic_inputs(seed, nc, n_rays, nonfinite=False)
    raw, rays = c["raw"], c["rays"]
    rng = np.random.default_rng(seed + 1)
    for r in range(8, min(40, n_rays)):                          # empty space with one to three occupied intervals
        raw[r, :, 3] = -5.0
        raw[r, rng.integers(0, nc, 1 + r % 3), 3] = rng.uniform(0.5, 40.0)
    raw[8, :, 3] = -5.0
    raw[8, 0, 3] = 50.0                                          # everything in weights[0], which the pdf leaves out
    raw[9, :, 3] = -5.0
    raw[9, nc - 1, 3] = 50.0
    finite = np.ones(n_rays, bool)
    if nonfinite:
        for j, r in enumerate(range(40, min(46, n_rays))):
            raw[r, (0, nc // 2, nc - 1)[j % 3], 3] = NONFINITE[j % 3] if j < 3 else np.nan
            finite[r] = False
    return dict(raw=raw, rays=rays, finite=finite)
