"""Restatements of the phased foveated density entry points and of adanerf_temporal_resolve_sparse (include/adanerf_hip.h), and the inputs
their tests use -- held apart from the library, so that the reference is never the code under test.

phase_of is the 64-phase cycle; mask_phased the mask rule by brute force (the smallest stride over every pixel of the box, as
tests/density_reference.py does it, with the lattice moved by the phase); fill_phased the reconstruction with every step one float32
operation; sparse_f32 the resolve operation by operation in numpy float32 (every numpy float32 array operation is one rounded fp32
operation), the clamp's minimum and maximum those of tests/temporal_reference.py.  The GPU tests ask for equality with these.  sparse_f64
is the resolve in float64: tests/test_sparse_temporal_cpu.py records how far the two are apart.

The rays, poses, depth scene and motions are those of tests/reproject_reference.py, the colours those of tests/temporal_reference.py."""
import collections

import numpy as np

import density_reference as DR
import reproject_reference as RR
import temporal_reference as TR
import upsample_reference as UR

F32 = np.float32
CLAMP = TR.CLAMP
ALPHA, DEPTH_TOL, ACC_MIN = TR.ALPHA, TR.DEPTH_TOL, TR.ACC_MIN
TEST_TOL = UR.TEST_TOL      # the depth tolerance of the GPU tests' geometric cases, for upsample_reference's reasons
SEED = 3
SIZES = [(48, 40), (37, 29), (64, 1), (1, 1)]
# the mask of the resolve tests: the gaze off the centre, so that the rings of strides 4 and 8 cross the depth scene's box
GAZE, SPEC = (0.31, 0.72), "4:1,9:2,15:4,8"
FOREIGN = 3                 # the byte planted outside {0, 2, 4, 8}

Result = collections.namedtuple("Result", "rgb depth count rgba8 mask rejected tap accepted live zp zlo zhi hd")


# ---- the cycle, the mask, the cell, the fill -------------------------------------------------------------

def phase_of(k):
    """(phase_x, phase_y) of frame k: the base-4 digits of k mod 64 place bit i of either phase"""
    k %= 64
    bx, by = (0, 1, 1, 0), (0, 1, 0, 1)
    d = [(k >> (2 * i)) & 3 for i in range(3)]
    return sum(bx[d[i]] << i for i in range(3)), sum(by[d[i]] << i for i in range(3))


def mask_phased(w, h, gaze, radius_px, stride, phase):
    """[h*w] uint8: 0 where some level L has the pixel on its lattice ((x - phase_x) mod L == 0, y alike) and the box of L - 1 pixels
    around the pixel (clipped) holds a stride <= L; the pixel's own stride elsewhere"""
    s = DR.stride_map(w, h, gaze, radius_px, stride)
    out = s.astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    for L in DR.LEVELS:
        r = L - 1
        pad = np.full((h + 2 * r, w + 2 * r), 99, np.int64)      # outside the frame: the box is clipped
        pad[r:r + h, r:r + w] = s
        box_min = np.min([pad[dy:dy + h, dx:dx + w] for dy in range(2 * r + 1) for dx in range(2 * r + 1)], axis=0)      # every pixel of the box
        out[((x - phase[0]) % L == 0) & ((y - phase[1]) % L == 0) & (box_min <= L)] = 0
    return out.reshape(-1)


def axis(c, phase, s, n):
    """(taps, m) of one axis of the cell of a pixel with byte s: taps () none, (c0,) one, (c0, c1) two; m the numerator of c1's weight"""
    m = (c - phase) % s
    lo, hi = c - m, c - m + s
    if m == 0:
        return (lo,), 0
    if lo >= 0 and hi < n:
        return (lo, hi), m
    if lo >= 0:
        return (lo,), m
    if hi < n:
        return (hi,), m
    return (), m


def used_corners(x, y, s, w, h, phase):
    """the distinct corner pixels as flat indices; [] where an axis has no tap (a frame narrower than the stride)"""
    xs, ys = axis(x, phase[0], s, w)[0], axis(y, phase[1], s, h)[0]
    return sorted({yy * w + xx for yy in ys for xx in xs})


def _blend(img, w, s, xs, mx, ys, my):
    fx, fy = F32(mx) / F32(s), F32(my) / F32(s)
    row = lambda yy: img[yy * w + xs[0]] if len(xs) == 1 else DR._lerp(img[yy * w + xs[0]], img[yy * w + xs[1]], fx)
    top = row(ys[0])
    return top if len(ys) == 1 else DR._lerp(top, row(ys[1]), fy)


def fill_phased(mask, w, h, phase, rgb, depth=None, acc=None, rgba8=None):
    """(rgb, depth, acc, rgba8, unfilled) after adanerf_fill_density_phased: tests/density_reference.py's fill with the cells of the phase"""
    mask = np.asarray(mask, np.uint8).reshape(-1)
    src = [np.asarray(rgb, F32).reshape(h * w, 3), None if depth is None else np.asarray(depth, F32).reshape(-1),
           None if acc is None else np.asarray(acc, F32).reshape(-1)]
    out = [None if a is None else a.copy() for a in src]
    out8 = None if rgba8 is None else np.asarray(rgba8, np.uint8).reshape(h * w, 4).copy()
    unfilled = 0
    for p in np.flatnonzero((mask == 2) | (mask == 4) | (mask == 8)).tolist():
        s = int(mask[p])
        y, x = divmod(p, w)
        (xs, mx), (ys, my) = axis(x, phase[0], s, w), axis(y, phase[1], s, h)
        if not xs or not ys or any(mask[yy * w + xx] != 0 for yy in ys for xx in xs):
            unfilled += 1
            continue
        for a, o in zip(src, out):
            if a is not None:
                o[p] = _blend(a, w, s, xs, mx, ys, my)      # corners carry byte 0: never rewritten, src == out there
        if out8 is not None:
            out8[p] = DR.rgba8_of(out[0][p])
    return out[0], out[1], out[2], out8, unfilled


# ---- the resolve -------------------------------------------------------------------------------------------

def sparse(scene, w, h, camera_origin, mask, phase, cur_rgb, cur_depth, cur_acc, cur_pos, cur_rot, hist_rgb, hist_depth, hist_count, prev_pos, prev_rot,
           alpha=ALPHA, depth_tol=DEPTH_TOL, acc_min=ACC_MIN, flags=CLAMP, dtype=F32):
    """Passes A and B of the header in `dtype`.  hist_rgb None: no history.  Returns Result(rgb [n,3] float32, depth [n] float32, count [n]
    uint8, rgba8 [n,4] uint8, mask [n] uint8, rejected, tap [n] int64 (-1: outside the history), accepted [n] bool, live [n] bool, zp [n] or
    None, zlo / zhi [n]: the smallest / largest finite zp of the pixel's set Z (+inf / -inf: none), hd [n]: the history's depth at the tap)."""
    T = dtype
    n = w * h
    mask = np.asarray(mask, np.uint8).reshape(-1)
    rendered, rebuilt = mask == 0, np.isin(mask, (2, 4, 8))
    cur32 = np.ascontiguousarray(cur_rgb, F32).reshape(n, 3)
    cur = cur32.astype(T)
    nds, p = (RR.rays_f32 if T is F32 else RR.rays_f64)(scene, w, h, cur_pos, cur_rot)
    cp, R = np.asarray(cur_pos, F32).astype(T).reshape(3), np.asarray(cur_rot, F32).astype(T).reshape(9)
    o = np.broadcast_to(cp.reshape(1, 3), nds.shape) if camera_origin else p
    a, dm = np.asarray(cur_acc, F32).reshape(-1).astype(T), np.asarray(cur_depth, F32).reshape(-1).astype(T)
    have_hist = hist_rgb is not None
    zp = zlo = zhi = hd = None
    with np.errstate(all="ignore"):
        t = dm / a
        near = (a >= T(F32(acc_min))) & np.isfinite(t) & (t > 0)
        P = [o[:, k] + nds[:, k] * t for k in range(3)]
        qc = [P[k] - cp[k] for k in range(3)]
        zc_cur = np.where(near, -((R[2] * qc[0] + R[5] * qc[1]) + R[8] * qc[2]), T(np.inf))
        assert zc_cur.dtype == T
        tap = np.full(n, -1, np.int64)
        accepted = np.zeros(n, bool)
        live = np.zeros(n, bool)
        count = rendered.astype(np.int64)
        verdict = np.zeros(n, np.uint8)
        out = cur.copy()
        if have_hist:
            pp, Rp = np.asarray(prev_pos, F32).astype(T).reshape(3), np.asarray(prev_rot, F32).astype(T).reshape(9)
            # ---- pass A
            if hist_depth is not None:
                q = [P[k] - pp[k] for k in range(3)]
                z = -((Rp[2] * q[0] + Rp[5] * q[1]) + Rp[8] * q[2])
                zp = np.where(near & np.isfinite(z), z, T(np.inf))
                assert zp.dtype == T
            # ---- pass B, 3: previous camera
            q = [np.where(near, P[k] - pp[k], nds[:, k]) for k in range(3)]
            v = [(Rp[k] * q[0] + Rp[3 + k] * q[1]) + Rp[6 + k] * q[2] for k in range(3)]
            zc = -v[2]
            ok = (zc > 0) & np.isfinite(zc)
            focal = T(F32(TR.O.focal_from_fov(w, scene.fov)))
            u = (focal * v[0]) / zc + T(0.5) * T(w)
            vv = (focal * (-v[1])) / zc + T(0.5) * T(h)
            ok &= (u >= 0) & (u < T(w)) & (vv >= 0) & (vv < T(h))
            u, vv = np.where(ok, u, T(0.5)), np.where(ok, vv, T(0.5))
            tap = np.where(ok, np.floor(vv).astype(np.int64) * w + np.floor(u).astype(np.int64), -1)
            safe = np.maximum(tap, 0)
            accepted = ok & (rendered | rebuilt)
            # 4: disocclusion
            if hist_depth is not None:
                hd = np.asarray(hist_depth, F32).reshape(-1).astype(T)[safe]
                nb = UR._neighbourhood(zp, w, h, T(np.nan))      # NaN: no such pixel; zp itself is finite or +inf
                finite = np.isfinite(nb)
                zlo = np.min(np.where(finite, nb, T(np.inf)), axis=0)
                zhi = np.max(np.where(finite, nb, T(-np.inf)), axis=0)
                any_far = (nb == T(np.inf)).any(axis=0)
                for j in np.flatnonzero(rebuilt).tolist():      # the used corners, not the neighbourhood
                    y, x = divmod(j, w)
                    zs = zp[used_corners(x, y, int(mask[j]), w, h, phase)]
                    fin = zs[np.isfinite(zs)]
                    zlo[j], zhi[j] = (fin.min(), fin.max()) if fin.size else (T(np.inf), T(-np.inf))
                    any_far[j] = bool((zs == T(np.inf)).any())
                any_finite = zlo <= zhi
                tol = T(F32(depth_tol))
                in_range = any_finite & (zlo - tol * zlo <= hd) & (hd <= zhi + tol * zhi)
                accepted &= np.where(hd == T(np.inf), any_far, np.where(np.isfinite(hd), in_range, False))
            # 5: history colour
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
            # 6: clamp, rendered pixels only
            clamped = hst
            if flags & CLAMP:
                lo, hi = TR.neighbourhood_bounds(cur, w, h)
                clamped = TR.min_rule(TR.max_rule(hst, lo), hi)
            # 7: count
            hc = np.asarray(hist_count, np.uint8).reshape(-1).astype(np.int64)[safe]
            live = accepted & (hc >= 1)
            n_new = np.minimum(hc + 1, 255)
            inv = T(1) / n_new.astype(T)
            al = np.full(n, T(F32(alpha)), T)
            a_eff = np.where(inv > al, inv, al)      # fmaxf of two numbers
            count = np.where(rendered, np.where(live, n_new, 1), np.where(live, hc, 0))
            verdict = np.where(live, 1, np.where(accepted, 2, 0)).astype(np.uint8)
            # 8: blend
            blend = clamped + a_eff[:, None] * (cur - clamped)
            assert blend.dtype == T
            out = np.where((live & rendered)[:, None], blend, np.where(live[:, None], hst, cur))
    rgb = np.where(live[:, None], out.astype(F32), cur32)      # not live: the bits copied
    return Result(rgb, zc_cur.astype(F32), count.astype(np.uint8), TR.AR.rgba8_of(rgb), verdict, int(np.count_nonzero(verdict == 0)), tap, accepted, live,
                  zp, zlo, zhi, hd)


def sparse_f32(*args, **kw):
    """The definition."""
    return sparse(*args, dtype=F32, **kw)


def sparse_f64(*args, **kw):
    """The same in float64 (the colours too; they come back rounded to float32)."""
    return sparse(*args, dtype=np.float64, **kw)


# ---- the inputs of the tests ---------------------------------------------------------------------------------

def resolve_mask(w, h, phase, foreign=True):
    """the mask of the resolve tests at a phase, with one pixel given the byte FOREIGN on frames that have room for it"""
    radius, stride = DR.parse_spec(SPEC)
    m = mask_phased(w, h, (float(F32(GAZE[0] * w)), float(F32(GAZE[1] * h))), radius, stride, phase)
    if foreign and w * h >= 12:
        m[(h // 3) * w + (2 * w) // 3] = FOREIGN
    return m


def current_at(scene, w, h, mask, phase, seed=SEED):
    """the frame the stage is handed: tests/temporal_reference.py's current frame (far pixels of every kind, NaNs, both zeros), the pixels
    of byte 2, 4 and 8 rebuilt by fill_phased as adanerf_fill_density_phased leaves them: (rgb [n,3], depth [n], acc [n])"""
    rgb, dm, acc = TR.current_at(scene, w, h, seed)
    on = np.flatnonzero(np.asarray(mask) == 0)
    if on.size >= 8:      # among the rendered pixels, whatever the lattice left of the planted ones: a negative depth and both zeros
        dm[on[on.size // 2]] = F32(-2.5)
        dm[on[on.size // 3]], dm[on[on.size // 3 + 1]] = F32(-0.0), F32(0.0)
    return fill_phased(mask, w, h, phase, rgb, dm, acc)[:3]


def history_at(scene, w, h, camera_origin, seed=SEED):
    """tests/temporal_reference.py's history (the true surfaces of the depth scene at the source pose, colours of its own) with
    tests/upsample_reference.py's counts: every value, 0, 1, 254 and 255 planted.  (rgb, depth, count, pose)"""
    rgb, depth, _, pose = TR.history_at(scene, w, h, camera_origin, seed)
    return rgb, depth, UR.planted_counts(w * h), pose


# history depth, clamp
COMBOS = [(True, True), (False, True), (True, False), (False, False)]


def geometric_cases():
    """(motion, phase, with_depth, clamp) of every call the GPU tests compare at a size: every motion x COMBOS, the 64 phases taken in
    turn from one that is not (0, 0)"""
    turn = 5
    for motion in RR.MOTIONS:
        for with_depth, clamp in COMBOS:
            yield motion, phase_of(turn), with_depth, clamp
            turn += 7      # 7 and 64 are coprime: 28 distinct phases
