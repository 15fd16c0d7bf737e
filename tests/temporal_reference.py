"""Restatements of adanerf_temporal_resolve (include/adanerf_hip.h) and the inputs its tests use -- held apart from the library, so that
the reference is never the code under test.

temporal_f32 is the definition operation by operation in numpy float32 (every numpy float32 array operation is one rounded fp32
operation, which is what the kernel's __fmul_rn / __fadd_rn / __fsub_rn / IEEE division are); the minimum and maximum of the clamp are
restated in integers (a NaN is skipped, -0 orders below +0), never through numpy's own minimum / maximum.  The GPU tests ask for
equality with it.  temporal_f64 is the same in float64: the tests' inputs must be such that the two agree on which pixels are accepted
and on the nearest tap nearly everywhere, which is a condition on the inputs, checked in tests/test_temporal_cpu.py.

The rays, poses, depth scene, motions and sizes are those of tests/reproject_reference.py."""
import collections

import numpy as np

import adanerf_oracle as O
import antialias_reference as AR
import reproject_reference as RR

F32 = np.float32
CLAMP = 1                     # ADANERF_TEMPORAL_CLAMP
ALPHA, DEPTH_TOL = 0.1, 0.02  # the hosts' defaults
ACC_MIN = RR.ACC_MIN

Result = collections.namedtuple("Result", "rgb depth count rgba8 mask rejected tap accepted")


# ---- the order of the clamp --------------------------------------------------------------------------

def _key(a):
    """floats as sign-magnitude integers: the order of the reals, with -0 below +0"""
    if a.dtype == F32:
        b = a.view(np.int32)
        return b ^ ((b >> 31) & np.int32(0x7FFFFFFF))
    b = a.view(np.int64)
    return b ^ ((b >> 63) & np.int64(0x7FFFFFFFFFFFFFFF))


def min_rule(a, b):
    """a NaN is skipped (both NaN: a NaN); otherwise the smaller by _key"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(_key(b) < _key(a), b, a)))


def max_rule(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(_key(b) > _key(a), b, a)))


def neighbourhood_bounds(cur, w, h):
    """(lo, hi) [n,3]: minimum / maximum of cur over the pixels of each pixel's 3 x 3 neighbourhood that exist, by the rules above"""
    T = cur.dtype.type
    pad = np.full((h + 2, w + 2, 3), np.nan, cur.dtype)
    pad[1:-1, 1:-1] = cur.reshape(h, w, 3)
    lo = np.full((h, w, 3), np.nan, cur.dtype)
    hi = lo.copy()
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            nb = pad[dy:dy + h, dx:dx + w]
            lo, hi = min_rule(lo, nb), max_rule(hi, nb)
    assert lo.dtype.type is T
    return lo.reshape(-1, 3), hi.reshape(-1, 3)


# ---- the definition ------------------------------------------------------------------------------------

def temporal(scene, w, h, camera_origin, cur_rgb, cur_depth, cur_acc, cur_pos, cur_rot, hist_rgb, hist_depth, hist_count, prev_pos, prev_rot,
             alpha=ALPHA, depth_tol=DEPTH_TOL, acc_min=ACC_MIN, flags=CLAMP, dtype=F32):
    """Steps 1 to 8 of the header in `dtype`.  hist_rgb None: no history.  Returns Result(rgb [n,3] float32, depth [n] float32,
    count [n] uint8, rgba8 [n,4] uint8, mask [n] uint8, rejected, tap [n] int64: the nearest tap of a pixel that lands inside the
    history, -1 otherwise, accepted [n] bool)."""
    T = dtype
    n = w * h
    cur32 = np.ascontiguousarray(cur_rgb, F32).reshape(n, 3)
    cur = cur32.astype(T)
    nds, p = (RR.rays_f32 if T is F32 else RR.rays_f64)(scene, w, h, cur_pos, cur_rot)
    cp, R = np.asarray(cur_pos, F32).astype(T).reshape(3), np.asarray(cur_rot, F32).astype(T).reshape(9)
    o = np.broadcast_to(cp.reshape(1, 3), nds.shape) if camera_origin else p
    a, dm = np.asarray(cur_acc, F32).reshape(-1).astype(T), np.asarray(cur_depth, F32).reshape(-1).astype(T)
    with np.errstate(all="ignore"):
        t = dm / a
        near = (a >= T(acc_min)) & np.isfinite(t) & (t > 0)
        P = [o[:, k] + nds[:, k] * t for k in range(3)]
        qc = [P[k] - cp[k] for k in range(3)]
        zc_cur = np.where(near, -((R[2] * qc[0] + R[5] * qc[1]) + R[8] * qc[2]), T(np.inf))
        assert zc_cur.dtype == T
        tap = np.full(n, -1, np.int64)
        accepted = np.zeros(n, bool)
        count = np.ones(n, np.int64)
        out = cur.copy()
        if hist_rgb is not None:
            pp, Rp = np.asarray(prev_pos, F32).astype(T).reshape(3), np.asarray(prev_rot, F32).astype(T).reshape(9)
            q = [np.where(near, P[k] - pp[k], nds[:, k]) for k in range(3)]
            v = [(Rp[k] * q[0] + Rp[3 + k] * q[1]) + Rp[6 + k] * q[2] for k in range(3)]
            zc = -v[2]
            ok = (zc > 0) & np.isfinite(zc)
            focal = T(F32(O.focal_from_fov(w, scene.fov)))
            u = (focal * v[0]) / zc + T(0.5) * T(w)
            vv = (focal * (-v[1])) / zc + T(0.5) * T(h)
            ok &= (u >= 0) & (u < T(w)) & (vv >= 0) & (vv < T(h))
            u, vv = np.where(ok, u, T(0.5)), np.where(ok, vv, T(0.5))
            tap = np.where(ok, np.floor(vv).astype(np.int64) * w + np.floor(u).astype(np.int64), -1)
            safe = np.maximum(tap, 0)
            accepted = ok.copy()
            if hist_depth is not None:
                hd = np.asarray(hist_depth, F32).reshape(-1).astype(T)[safe]
                accepted &= np.where(near, np.isfinite(hd) & (np.abs(zc - hd) <= T(F32(depth_tol)) * zc), hd == T(np.inf))
            fx, fy = u - T(0.5), vv - T(0.5)
            x0, y0 = np.floor(fx), np.floor(fy)
            wx, wy = (fx - x0)[:, None], (fy - y0)[:, None]
            xa, xb = np.clip(x0.astype(np.int64), 0, w - 1), np.clip(x0.astype(np.int64) + 1, 0, w - 1)
            ya, yb = np.clip(y0.astype(np.int64), 0, h - 1), np.clip(y0.astype(np.int64) + 1, 0, h - 1)
            hist = np.ascontiguousarray(hist_rgb, F32).reshape(h, w, 3).astype(T)
            c00, c01, c10, c11 = hist[ya, xa], hist[ya, xb], hist[yb, xa], hist[yb, xb]
            top = c00 + wx * (c01 - c00)
            bot = c10 + wx * (c11 - c10)
            hst = top + wy * (bot - top)
            assert hst.dtype == T and wx.dtype == T
            if flags & CLAMP:
                lo, hi = neighbourhood_bounds(cur, w, h)
                hst = min_rule(max_rule(hst, lo), hi)
            a_eff = np.full(n, T(F32(alpha)), T)
            if hist_count is not None:
                count = np.where(accepted, np.minimum(np.asarray(hist_count, np.uint8).reshape(-1).astype(np.int64)[safe] + 1, 255), 1)
                inv = T(1) / count.astype(T)
                a_eff = np.where(inv > a_eff, inv, a_eff)      # fmaxf of two numbers
            blend = hst + a_eff[:, None] * (cur - hst)
            assert blend.dtype == T
            out = np.where(accepted[:, None], blend, cur)
    rgb = np.where(accepted[:, None], out.astype(F32), cur32)      # a rejected pixel: the bits copied
    mask = accepted.astype(np.uint8)
    return Result(rgb, zc_cur.astype(F32), count.astype(np.uint8), AR.rgba8_of(rgb), mask, int(np.count_nonzero(mask == 0)), tap, accepted)


def temporal_f32(*args, **kw):
    """The definition."""
    return temporal(*args, dtype=F32, **kw)


def temporal_f64(*args, **kw):
    """The same in float64 (the colours too; they come back rounded to float32)."""
    return temporal(*args, dtype=np.float64, **kw)


# ---- the inputs of the tests ---------------------------------------------------------------------------

def colours(w, h, seed, planted=True):
    """[n,3] float32 in about -0.5 .. 1.5 (values outside [0, 1] are common); planted: NaNs (the default quiet NaN), +0 / -0 pairs side
    by side and one pixel whose whole neighbourhood is NaN.  No infinities: what an invalid operation (inf - inf) returns is a NaN
    whose sign is the platform's, and that would make colour BITS a demand on the host, not on the kernel."""
    rng = np.random.default_rng(seed + 104729 * w + 31 * h)
    n = w * h
    c = (rng.random((n, 3)) * 2.0 - 0.5).astype(F32)
    if planted and n >= 12:
        k = rng.permutation(n)[:max(6, n // 12)]
        for j, i in enumerate(k):
            kind = j % 4
            if kind == 0:
                c[i, j % 3] = F32(np.nan)
            elif kind == 1:
                c[i] = F32(np.nan)
            elif kind == 2:
                c[i, 0], c[(i + 1) % n, 0] = F32(0.0), F32(-0.0)
            else:
                c[i], c[(i + 1) % n] = F32(-0.0), F32(0.0)
        if w >= 5 and h >= 5:
            c.reshape(h, w, 3)[h // 2 - 1:h // 2 + 2, w // 2 - 1:w // 2 + 2, 1] = F32(np.nan)      # a whole neighbourhood in one channel
    return c


def history_at(scene, w, h, camera_origin, seed, counts="ramp"):
    """The history triple a first call (no history) at the source pose of tests/reproject_reference.py leaves over its depth scene, with
    planted colours of its own: (rgb [n,3], depth [n], count [n] uint8, pose).  counts: "ramp" 1, 2, ... with 254 and 255 among them."""
    _, dm, acc, _ = RR.depth_scene(w, h, seed)
    pos, rot = RR.src_pose(scene)
    first = temporal_f32(scene, w, h, camera_origin, colours(w, h, seed + 50), dm, acc, pos, rot, None, None, None, None, None)
    n = w * h
    count = ((np.arange(n) * 7) % 255 + 1).astype(np.uint8)      # 1 .. 255, each value several times on a frame of a few hundred pixels
    if n >= 4:
        count[[0, n // 2]] = 254
        count[[1, n - 1]] = 255
    return first.rgb, first.depth, count, (pos, rot)


def current_at(scene, w, h, seed):
    """the new frame: another depth scene of the same kind (far pixels of every kind planted) and planted colours"""
    _, dm, acc, _ = RR.depth_scene(w, h, seed + 1)
    return colours(w, h, seed + 90), dm, acc
