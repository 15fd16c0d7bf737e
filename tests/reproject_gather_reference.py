"""Restatements of adanerf_reproject_gather (include/adanerf_hip.h) -- held apart from the library, so that the reference is never the
code under test.

gather_f32 is the definition operation by operation in numpy float32 (every numpy float32 array operation is one rounded fp32
operation, which is what the kernels' __fmul_rn / __fadd_rn / __fsub_rn / IEEE division are), over the float64 pixel-ray table as the
kernels' gen_ray computes it.  The GPU tests ask for equality with it.  gather_f64 is the same geometry in float64: the tests' inputs
must be such that the two agree on the mask and on the final tap nearly everywhere, which is a condition on the inputs, checked in
tests/test_reproject_gather_cpu.py.

The rays, poses, depth scene, motions and sizes are those of tests/reproject_reference.py; the colours those of
tests/temporal_reference.py."""
import collections

import numpy as np

import adanerf_oracle as O
import antialias_reference as AR
from reproject_reference import ACC_MIN, HOLE, MOTIONS, SIZES, depth_scene, moved, rays_f32, rays_f64, src_pose      # noqa: F401
from temporal_reference import colours      # noqa: F401

F32 = np.float32
GUESS = 1                     # ADANERF_GATHER_GUESS
ITERATIONS, DEPTH_TOL = 4, 0.05      # the hosts' defaults (profiles/reproject_gather_measured.md)
GPU_SIZES = SIZES + [(33, 9)]      # one pixel over a 32 x 8 tile each way

Result = collections.namedtuple("Result", "rgb rgba8 depth mask holes tap alive consistent")


def surfaces(scene, w, h, camera_origin, depth, acc, pos, rot, acc_min=ACC_MIN, dtype=F32):
    """Step 1 (pass A): (S [n,3], zs [n]) per source pixel; zs = +inf marks a far pixel, whose S is never read."""
    T = dtype
    nds, p = (rays_f32 if T is F32 else rays_f64)(scene, w, h, pos, rot)
    sp, R = np.asarray(pos, F32).astype(T).reshape(3), np.asarray(rot, F32).astype(T).reshape(9)
    o = np.broadcast_to(sp.reshape(1, 3), nds.shape) if camera_origin else p
    a, dm = np.asarray(acc, F32).reshape(-1).astype(T), np.asarray(depth, F32).reshape(-1).astype(T)
    with np.errstate(all="ignore"):
        t = dm / a
        near = (a >= T(acc_min)) & np.isfinite(t) & (t > 0)
        S = np.stack([o[:, k] + nds[:, k] * t for k in range(3)], axis=1)
        q = [S[:, k] - sp[k] for k in range(3)]
        zs = np.where(near, -((R[2] * q[0] + R[5] * q[1]) + R[8] * q[2]), T(np.inf))
    assert S.dtype == T and zs.dtype == T
    return S, zs


def gather(scene, w, h, camera_origin, src_rgb, depth, acc, s_pos, s_rot, d_pos, d_rot, acc_min=ACC_MIN, depth_tol=DEPTH_TOL, iterations=ITERATIONS,
           hole_rgba8=HOLE, flags=0, dtype=F32):
    """Steps 1 to 5 of the header in `dtype`.  Returns Result(rgb [n,3] float32, rgba8 [n,4] uint8, depth [n] float32, mask [n] uint8, holes,
    tap [n] int64: the final tap (of a dead pixel: the last one it had), alive [n] bool, consistent [n] bool)."""
    T = dtype
    n = w * h
    S, zs = surfaces(scene, w, h, camera_origin, depth, acc, s_pos, s_rot, acc_min, T)
    d, _ = (rays_f32 if T is F32 else rays_f64)(scene, w, h, d_pos, d_rot)
    sp, Rs = np.asarray(s_pos, F32).astype(T).reshape(3), np.asarray(s_rot, F32).astype(T).reshape(9)
    dp, Rd = np.asarray(d_pos, F32).astype(T).reshape(3), np.asarray(d_rot, F32).astype(T).reshape(9)
    focal = T(F32(O.focal_from_fov(w, scene.fov)))      # adanerf_info.focal: the float64 focal length as fp32
    tap = np.arange(n, dtype=np.int64)
    alive = np.ones(n, bool)
    u, vv = np.full(n, T(0.5), T), np.full(n, T(0.5), T)
    zc = np.zeros(n, T)
    P = np.zeros((n, 3), T)
    est_near = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            Sk, zk = S[tap], zs[tap]
            near = zk != T(np.inf)
            s = ((Sk[:, 0] - dp[0]) * d[:, 0] + (Sk[:, 1] - dp[1]) * d[:, 1]) + (Sk[:, 2] - dp[2]) * d[:, 2]
            ok = ~near | (np.isfinite(s) & (s > 0))
            Pk = np.stack([dp[k] + d[:, k] * s for k in range(3)], axis=1)
            q = [np.where(near, Pk[:, k] - sp[k], d[:, k]) for k in range(3)]
            v = [(Rs[k] * q[0] + Rs[3 + k] * q[1]) + Rs[6 + k] * q[2] for k in range(3)]
            z = -v[2]
            uk = (focal * v[0]) / z + T(0.5) * T(w)
            vk = (focal * (-v[1])) / z + T(0.5) * T(h)
            ok &= (z > 0) & np.isfinite(z) & (uk >= 0) & (uk < T(w)) & (vk >= 0) & (vk < T(h))
            assert s.dtype == T and uk.dtype == T and Pk.dtype == T
            alive &= ok      # a dead pixel keeps what it had
            tap = np.where(alive, np.floor(np.where(alive, vk, 0)).astype(np.int64) * w + np.floor(np.where(alive, uk, 0)).astype(np.int64), tap)
            u, vv, zc = np.where(alive, uk, u), np.where(alive, vk, vv), np.where(alive, z, zc)
            P = np.where(alive[:, None], Pk, P)
            est_near = np.where(alive, near, est_near)
        zt = zs[tap]
        tap_near = zt != T(np.inf)
        consistent = np.where(est_near, tap_near & (np.abs(zc - zt) <= T(F32(depth_tol)) * zc), ~tap_near)
        qd = [P[:, k] - dp[k] for k in range(3)]
        zd = np.where(est_near, -((Rd[2] * qd[0] + Rd[5] * qd[1]) + Rd[8] * qd[2]), T(np.inf))
        # step 5: the bilinear tap of the source colour at the last (u, vv)
        fx, fy = u - T(0.5), vv - T(0.5)
        x0, y0 = np.floor(fx), np.floor(fy)
        wx, wy = (fx - x0)[:, None], (fy - y0)[:, None]
        xa, xb = np.clip(x0.astype(np.int64), 0, w - 1), np.clip(x0.astype(np.int64) + 1, 0, w - 1)
        ya, yb = np.clip(y0.astype(np.int64), 0, h - 1), np.clip(y0.astype(np.int64) + 1, 0, h - 1)
        src = np.ascontiguousarray(src_rgb, F32).reshape(h, w, 3).astype(T)
        c00, c01, c10, c11 = src[ya, xa], src[ya, xb], src[yb, xa], src[yb, xb]
        top = c00 + wx * (c01 - c00)
        bot = c10 + wx * (c11 - c10)
        col = top + wy * (bot - top)
        assert col.dtype == T and zd.dtype == T
    mask = np.where(alive & consistent, 1, np.where(alive & bool(flags & GUESS), 2, 0)).astype(np.uint8)
    shown = mask > 0
    rgb = np.where(shown[:, None], col.astype(F32), F32(0))
    hole_px = np.frombuffer(np.uint32(hole_rgba8).tobytes(), np.uint8)
    rgba8 = np.where(shown[:, None], AR.rgba8_of(rgb), hole_px[None, :]).astype(np.uint8)
    out_depth = np.where(shown, zd.astype(F32), F32(0))
    return Result(rgb, rgba8, out_depth, mask, int(np.count_nonzero(mask == 0)), tap, alive, consistent & alive)


def gather_f32(*args, **kw):
    """The definition."""
    return gather(*args, dtype=F32, **kw)


def gather_f64(*args, **kw):
    """The same geometry in float64 (the colours too; they come back rounded to float32)."""
    return gather(*args, dtype=np.float64, **kw)
