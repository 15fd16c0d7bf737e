"""Restatements of adanerf_temporal_upsample (include/adanerf_hip.h) and the inputs its tests use -- held apart from the library, so that
the reference is never the code under test.

upsample_f32 is the definition operation by operation in numpy float32 (every numpy float32 array operation is one rounded fp32
operation); the clamp's minimum and maximum are tests/temporal_reference.py's min_rule / max_rule.  The GPU tests ask for equality with
it.  upsample_f64 is the same in float64: the tests' inputs must be such that the two agree on the nearest sample, the tap and the mask
nearly everywhere, which is a condition on the inputs, checked in tests/test_upsample_cpu.py.

The rays, poses, depth scene, motions and sizes are those of tests/reproject_reference.py; the colours those of
tests/temporal_reference.py; the ray table with an offset that of tests/antialias_reference.py."""
import collections

import numpy as np

import adanerf_oracle as O
import antialias_reference as AR
import reproject_reference as RR
import temporal_reference as TR

F32 = np.float32
CLAMP = TR.CLAMP
ALPHA, DEPTH_TOL = TR.ALPHA, TR.DEPTH_TOL      # the hosts' defaults
ACC_MIN = RR.ACC_MIN
# The depth tolerance and seed of the GPU tests' geometric cases.  The neighbourhood test accepts whatever the range of depths over 3 x 3
# render pixels explains, and on the 16 x 12 frame the hosts' 2 % accepts all but the planted far pixels of the small moves (under 5 %
# rejected); at 0.2 % every moved case but sees_none both accepts and rejects at least 5 % of its pixels at every size, scale and offset
# (7.9 % at the least: 16 x 12, s = 2, forward).  tests/test_upsample_cpu.py holds that condition.
TEST_TOL = 0.002
SEED = 1
SCALES = {(16, 12): (1, 2, 3, 4), (97, 61): (2, 3), (64, 1): (2,), (1, 1): (1, 4)}      # render size -> scales of the GPU tests
ODD_OFFSETS = [(0.37, -0.81), (1.0, -1.0), (0.0, 0.0)]                                   # beside the grid's own

Result = collections.namedtuple("Result", "rgb depth count rgba8 mask rejected tap accepted ix iy inside k")


def rays(scene, w, h, pos, rot, dx, dy, dtype):
    """(nds [n,3], p [n,3]) of the w x h ray generator with the offset (dx, dy) applied as adanerf_set_pixel_offset defines, in dtype"""
    if dtype is F32:
        r = AR.rays(scene, w, h, pos, rot, dx, dy)
        return r[:, 4:7], r[:, 0:3]
    focal = O.focal_from_fov(w, scene.fov)
    x_dist = np.tan(scene.fov / 2) * focal
    y_dist = x_dist * (h / w)
    x_pp, y_pp = x_dist / (w / 2), y_dist / (h / 2)
    row, col = np.divmod(np.arange(w * h), w)
    v = np.stack([-(x_dist - x_pp / 2) + x_pp * (col + float(F32(dx))), -(-(y_dist - y_pp / 2) + y_pp * (row + float(F32(dy)))),
                  np.full(w * h, -focal)], axis=1)
    v /= np.linalg.norm(v, axis=1)[:, None]
    rot = np.asarray(rot, np.float64).reshape(3, 3)
    pos = np.asarray(pos, np.float64).reshape(3)
    nds = v @ rot.T
    q = pos - np.asarray(scene.view_cell_center, np.float64)
    udot = nds @ q
    delta = udot * udot - (q @ q - RR._rad2(scene))
    dist = -udot + np.sqrt(np.maximum(delta, 0.0))
    return nds, pos[None, :] + nds * dist[:, None]


def nearest_sample(n_out, s, d, n, T=F32):
    """step 1 along one axis for X = 0 .. n_out - 1: (ix int64, e: the sample's distance from the output pixel's centre, in T)"""
    X = np.arange(n_out).astype(T)
    c = (X + T(0.5)) / T(s) - T(F32(d))
    ix = np.clip(np.floor(c).astype(np.int64), 0, n - 1)
    e = ((ix.astype(T) + T(0.5)) + T(F32(d))) * T(s) - (X + T(0.5))
    assert c.dtype == T and e.dtype == T
    return ix, e


def _neighbourhood(img, w, h, fill):
    """the 9 shifted copies [9, h*w, ...] of a [h*w, ...] image, `fill` where the neighbour does not exist"""
    a = img.reshape((h, w) + img.shape[1:])
    pad = np.full((h + 2, w + 2) + img.shape[1:], fill, img.dtype)
    pad[1:-1, 1:-1] = a
    return np.stack([pad[dy:dy + h, dx:dx + w].reshape(img.shape) for dy in (0, 1, 2) for dx in (0, 1, 2)])


def upsample(scene, w, h, s, camera_origin, cur_rgb, cur_depth, cur_acc, cur_dx, cur_dy, cur_pos, cur_rot, hist_rgb, hist_depth, hist_count,
             prev_pos, prev_rot, alpha=ALPHA, depth_tol=DEPTH_TOL, acc_min=ACC_MIN, flags=CLAMP, dtype=F32):
    """Passes A and B of the header in `dtype`.  hist_rgb None: no history.  Returns Result(rgb [N,3] float32, depth [N] float32, count [N]
    uint8, rgba8 [N,4] uint8, mask [N] uint8, rejected, tap [N] int64 (-1: outside the history), accepted [N] bool, ix / iy [W] / [H]
    int64, inside [N] bool, k [N] in dtype), N = s w s h."""
    T = dtype
    W, H = s * w, s * h
    n, N = w * h, W * H
    cur32 = np.ascontiguousarray(cur_rgb, F32).reshape(n, 3)
    cp, R = np.asarray(cur_pos, F32).astype(T).reshape(3), np.asarray(cur_rot, F32).astype(T).reshape(9)
    a_lo, dm_lo = np.asarray(cur_acc, F32).reshape(-1).astype(T), np.asarray(cur_depth, F32).reshape(-1).astype(T)
    have_hist = hist_rgb is not None
    with np.errstate(all="ignore"):
        t_lo = dm_lo / a_lo
        near_lo = (a_lo >= T(F32(acc_min))) & np.isfinite(t_lo) & (t_lo > 0)
        # ---- pass A
        zp = None
        if have_hist and hist_depth is not None:
            pp, Rp = np.asarray(prev_pos, F32).astype(T).reshape(3), np.asarray(prev_rot, F32).astype(T).reshape(9)
            nds, p = rays(scene, w, h, cur_pos, cur_rot, cur_dx, cur_dy, T)
            o = np.broadcast_to(cp.reshape(1, 3), nds.shape) if camera_origin else p
            q = [(o[:, k] + nds[:, k] * t_lo) - pp[k] for k in range(3)]
            z = -((Rp[2] * q[0] + Rp[5] * q[1]) + Rp[8] * q[2])
            zp = np.where(near_lo & np.isfinite(z), z, T(np.inf))
            assert zp.dtype == T
        # ---- pass B, 1: sample
        ix, ex = nearest_sample(W, s, cur_dx, w, T)
        iy, ey = nearest_sample(H, s, cur_dy, h, T)
        i = (iy[:, None] * w + ix[None, :]).reshape(-1)
        EX, EY = np.broadcast_to(ex[None, :], (H, W)).reshape(-1), np.broadcast_to(ey[:, None], (H, W)).reshape(-1)
        k = np.maximum(T(0), T(1) - np.abs(EX)) * np.maximum(T(0), T(1) - np.abs(EY))
        inside = (np.abs(EX) <= T(0.5)) & (np.abs(EY) <= T(0.5))
        cur_bits = cur32[i]
        cur = cur_bits.astype(T)
        # 2: surface and own depth
        nds, p = rays(scene, W, H, cur_pos, cur_rot, 0.0, 0.0, T)
        o = np.broadcast_to(cp.reshape(1, 3), nds.shape) if camera_origin else p
        t, near = t_lo[i], near_lo[i]
        P = [o[:, c] + nds[:, c] * t for c in range(3)]
        qc = [P[c] - cp[c] for c in range(3)]
        zc_cur = np.where(near, -((R[2] * qc[0] + R[5] * qc[1]) + R[8] * qc[2]), T(np.inf))
        tap = np.full(N, -1, np.int64)
        accepted = np.zeros(N, bool)
        live = np.zeros(N, bool)
        count = inside.astype(np.int64)
        mask = np.zeros(N, np.uint8)
        out = cur.copy()
        if have_hist:
            # 3: previous camera
            pp, Rp = np.asarray(prev_pos, F32).astype(T).reshape(3), np.asarray(prev_rot, F32).astype(T).reshape(9)
            q = [np.where(near, P[c] - pp[c], nds[:, c]) for c in range(3)]
            v = [(Rp[c] * q[0] + Rp[3 + c] * q[1]) + Rp[6 + c] * q[2] for c in range(3)]
            zc = -v[2]
            ok = (zc > 0) & np.isfinite(zc)
            focal = T(F32(O.focal_from_fov(W, scene.fov)))
            u = (focal * v[0]) / zc + T(0.5) * T(W)
            vv = (focal * (-v[1])) / zc + T(0.5) * T(H)
            ok &= (u >= 0) & (u < T(W)) & (vv >= 0) & (vv < T(H))
            u, vv = np.where(ok, u, T(0.5)), np.where(ok, vv, T(0.5))
            tap = np.where(ok, np.floor(vv).astype(np.int64) * W + np.floor(u).astype(np.int64), -1)
            safe = np.maximum(tap, 0)
            accepted = ok.copy()
            # 4: disocclusion
            if hist_depth is not None:
                hd = np.asarray(hist_depth, F32).reshape(-1).astype(T)[safe]
                nb = _neighbourhood(zp, w, h, T(np.nan))      # NaN: no such pixel; zp itself is finite or +inf
                finite = np.isfinite(nb)
                zmin = np.min(np.where(finite, nb, T(np.inf)), axis=0)[i]
                zmax = np.max(np.where(finite, nb, T(-np.inf)), axis=0)[i]
                any_finite, any_far = finite.any(axis=0)[i], (nb == T(np.inf)).any(axis=0)[i]
                tol = T(F32(depth_tol))
                in_range = any_finite & (zmin - tol * zmin <= hd) & (hd <= zmax + tol * zmax)
                accepted &= np.where(hd == T(np.inf), any_far, np.where(np.isfinite(hd), in_range, False))
            # 5: history colour
            fx, fy = u - T(0.5), vv - T(0.5)
            x0, y0 = np.floor(fx), np.floor(fy)
            wx, wy = (fx - x0)[:, None], (fy - y0)[:, None]
            xa, xb = np.clip(x0.astype(np.int64), 0, W - 1), np.clip(x0.astype(np.int64) + 1, 0, W - 1)
            ya, yb = np.clip(y0.astype(np.int64), 0, H - 1), np.clip(y0.astype(np.int64) + 1, 0, H - 1)
            hist = np.ascontiguousarray(hist_rgb, F32).reshape(H, W, 3).astype(T)
            c00, c01, c10, c11 = hist[ya, xa], hist[ya, xb], hist[yb, xa], hist[yb, xb]
            top = c00 + wx * (c01 - c00)
            bot = c10 + wx * (c11 - c10)
            hst = top + wy * (bot - top)
            assert hst.dtype == T
            # 6: clamp
            if flags & CLAMP:
                lo, hi = TR.neighbourhood_bounds(cur32.astype(T), w, h)
                hst = TR.min_rule(TR.max_rule(hst, lo[i]), hi[i])
            # 7: count
            a_eff = k * T(F32(alpha))
            if hist_count is not None:
                hc = np.asarray(hist_count, np.uint8).reshape(-1).astype(np.int64)[safe]
                live = accepted & (hc >= 1)
                n_new = np.minimum(hc + inside, 255)
                inv = T(1) / np.maximum(n_new, 1).astype(T)
                al = np.full(N, T(F32(alpha)), T)
                a_eff = k * np.where(inv > al, inv, al)      # fmaxf of two numbers
                count = np.where(live, n_new, inside.astype(np.int64))
                mask = np.where(live, 1, np.where(accepted, 2, 0)).astype(np.uint8)
            else:
                live = accepted.copy()
                count = (live | inside).astype(np.int64)
                mask = live.astype(np.uint8)
            # 8: blend
            blend = np.where((k > 0)[:, None], hst + a_eff[:, None] * (cur - hst), hst)
            assert blend.dtype == T
            out = np.where(live[:, None], blend, cur)
    rgb = np.where(live[:, None], out.astype(F32), cur_bits)      # not live: the bits copied
    return Result(rgb, zc_cur.astype(F32), count.astype(np.uint8), AR.rgba8_of(rgb), mask, int(np.count_nonzero(mask == 0)), tap, accepted, ix, iy,
                  inside, k)


def upsample_f32(*args, **kw):
    """The definition."""
    return upsample(*args, dtype=F32, **kw)


def upsample_f64(*args, **kw):
    """The same in float64 (the colours too; they come back rounded to float32)."""
    return upsample(*args, dtype=np.float64, **kw)


# ---- the inputs of the tests ---------------------------------------------------------------------------

def offsets_of(s):
    """the offsets a size's cases run: the grid's own and the odd ones"""
    return AR.subpixel_grid(s) + ODD_OFFSETS


# history depth, history count, clamp
COMBOS = [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)]


def geometric_cases(s):
    """(motion, offset, with_depth, with_count, clamp) of every call the GPU tests compare at scale s: every motion x COMBOS with the offsets
    taken in turn, then every offset on the lateral move with everything on"""
    offsets = offsets_of(s)
    turn = 0
    for motion in RR.MOTIONS:
        for combo in COMBOS:
            yield (motion, offsets[turn % len(offsets)]) + combo
            turn += 1
    for offset in offsets:
        yield ("lateral", offset, True, True, True)


def planted_counts(N):
    """[N] uint8: every value 0 .. 255 in turn, with 0, 1, 254 and 255 at fixed places on any frame of at least 4 pixels"""
    count = ((np.arange(N) * 7) % 256).astype(np.uint8)
    if N >= 4:
        count[[0, N // 2]] = (254, 0)
        count[[1, N - 1]] = (255, 1)
    return count


def history_at(scene, w, h, s, camera_origin, seed):
    """The history triple a first call (no history, pixel centres) at the source pose of tests/reproject_reference.py leaves over its depth
    scene with planted colours of its own: (rgb [N,3], depth [N], count [N] uint8 planted, pose)."""
    _, dm, acc, _ = RR.depth_scene(w, h, seed)
    pos, rot = RR.src_pose(scene)
    first = upsample_f32(scene, w, h, s, camera_origin, TR.colours(w, h, seed + 50), dm, acc, 0.0, 0.0, pos, rot, None, None, None, None, None)
    return first.rgb, first.depth, planted_counts(s * w * s * h), (pos, rot)


def current_at(scene, w, h, seed):
    """the new frame at the render size: another depth scene of the same kind (far pixels of every kind planted) and planted colours"""
    return TR.current_at(scene, w, h, seed)
