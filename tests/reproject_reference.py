"""Restatements of adanerf_reproject (include/adanerf_hip.h) and the inputs its tests use -- held apart from the library, so that the
reference is never the code under test.

reproject_f32 is the definition operation by operation in numpy float32 (every numpy float32 array operation is one rounded fp32
operation, which is what the kernel's __fmul_rn / __fadd_rn / IEEE division are), over the float64 pixel-ray table of
oracle/adanerf_oracle.py (generate_ray_directions), as the kernel's gen_ray computes it.  The GPU tests ask for equality with it.
reproject_f64 is the same geometry in float64: the tests' inputs must be such that the two agree on which source pixel wins nearly
everywhere (pixel-boundary and depth ties are rare), which is a condition on the inputs, checked in tests/test_reproject_cpu.py."""
import math

import numpy as np

import adanerf_oracle as O

F32 = np.float32
FILL = 1                      # ADANERF_REPROJECT_FILL
FAR_BITS = 0x7F800000         # +inf
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
ACC_MIN = 0.5
HOLE = 0x80FF40C0             # hole colour of the tests: bytes C0 40 FF 80


# ---- the pixel rays --------------------------------------------------------------------------------

def _rad2(scene):
    r2 = 0.0
    for s in scene.view_cell_size:      # the library holds the sizes in fp32 and sums the squares of their halves in float64
        r2 += (float(F32(s)) / 2.0) * (float(F32(s)) / 2.0)
    rad = math.sqrt(r2)
    return rad * rad


def rays_f32(scene, w, h, pos, rot):
    """k_common.hip.hpp gen_ray for every pixel: (nds [n,3], p [n,3]) in float32, n = h*w, from the float64 ray table"""
    d = O.generate_ray_directions(w, h, scene.fov)      # float64 arithmetic, cast to float32
    rot = np.asarray(rot, F32).reshape(9)
    pos = np.asarray(pos, F32).reshape(3)
    nds = np.stack([(rot[3 * i] * d[:, 0] + rot[3 * i + 1] * d[:, 1]) + rot[3 * i + 2] * d[:, 2] for i in range(3)], axis=1)
    c = np.asarray(scene.view_cell_center, F32)
    q = pos - c
    udot = (q[0] * nds[:, 0] + q[1] * nds[:, 1]) + q[2] * nds[:, 2]
    qq = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
    delta = udot * udot - (qq - F32(_rad2(scene)))
    dist = -udot + np.sqrt(np.maximum(delta, F32(0)))
    p = pos[None, :] + nds * dist[:, None]
    assert nds.dtype == F32 and p.dtype == F32
    return nds, p


def rays_f64(scene, w, h, pos, rot):
    focal = O.focal_from_fov(w, scene.fov)
    x_dist = np.tan(scene.fov / 2) * focal
    y_dist = x_dist * (h / w)
    x_pp, y_pp = x_dist / (w / 2), y_dist / (h / 2)
    row, col = np.divmod(np.arange(w * h), w)
    v = np.stack([-(x_dist - x_pp / 2) + x_pp * col, -(-(y_dist - y_pp / 2) + y_pp * row), np.full(w * h, -focal)], axis=1)
    v /= np.linalg.norm(v, axis=1)[:, None]
    rot = np.asarray(rot, np.float64).reshape(3, 3)
    pos = np.asarray(pos, np.float64).reshape(3)
    nds = v @ rot.T
    q = pos - np.asarray(scene.view_cell_center, np.float64)
    udot = nds @ q
    delta = udot * udot - (q @ q - _rad2(scene))
    dist = -udot + np.sqrt(np.maximum(delta, 0.0))
    return nds, pos[None, :] + nds * dist[:, None]


# ---- splat -----------------------------------------------------------------------------------------

def splat(scene, w, h, camera_origin, depth, acc, src_pos, src_rot, dst_pos, dst_rot, acc_min, dtype=F32):
    """Per source pixel: (ok: it lands inside the destination, pix: where, zc: its camera depth there, near).  dtype float32: the
    definition; float64: the same geometry."""
    T = dtype
    nds, p = (rays_f32 if T is F32 else rays_f64)(scene, w, h, src_pos, src_rot)
    o = np.broadcast_to(np.asarray(src_pos, T).reshape(1, 3), nds.shape) if camera_origin else p
    a, dm = np.asarray(acc, F32).reshape(-1).astype(T), np.asarray(depth, F32).reshape(-1).astype(T)
    dp, R = np.asarray(dst_pos, F32).astype(T).reshape(3), np.asarray(dst_rot, F32).astype(T).reshape(9)
    with np.errstate(all="ignore"):
        t = dm / a
        near = (a >= T(acc_min)) & np.isfinite(t) & (t > 0)
        q = [np.where(near, (o[:, k] + nds[:, k] * t) - dp[k], nds[:, k]) for k in range(3)]
        v = [(R[k] * q[0] + R[3 + k] * q[1]) + R[6 + k] * q[2] for k in range(3)]
        zc = -v[2]
        ok = (zc > 0) & np.isfinite(zc)
        focal = T(F32(O.focal_from_fov(w, scene.fov)))      # adanerf_info.focal: the float64 focal length as fp32
        u = (focal * v[0]) / zc + T(0.5) * T(w)
        vv = (focal * (-v[1])) / zc + T(0.5) * T(h)
        ok &= (u >= 0) & (u < T(w)) & (vv >= 0) & (vv < T(h))
        pix = np.where(ok, np.floor(np.where(ok, vv, 0)).astype(np.int64) * w + np.floor(np.where(ok, u, 0)).astype(np.int64), -1)
    assert zc.dtype == T and u.dtype == T
    return ok, pix, np.where(near, zc, T(np.inf)), near


def _resolve(w, h, winner, rank, zc_of_src, src_rgba, hole_rgba8, fill):
    """winner [n] source index or -1, rank [n] uint64 (0: none; larger = farther, unique): colour, depth, mask, holes"""
    n = w * h
    mask = (winner >= 0).astype(np.uint8)
    take = winner.copy()
    if fill:
        pad = np.zeros((h + 2, w + 2), np.uint64)
        pad[1:-1, 1:-1] = rank.reshape(h, w)
        widx = np.full((h + 2, w + 2), -1, np.int64)
        widx[1:-1, 1:-1] = winner.reshape(h, w)
        best, best_i = np.zeros((h, w), np.uint64), np.full((h, w), -1, np.int64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                r, i = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w], widx[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                better = r > best
                best, best_i = np.where(better, r, best), np.where(better, i, best_i)
        filled = (winner < 0) & (best_i.reshape(-1) >= 0)
        take = np.where(filled, best_i.reshape(-1), take)
        mask[filled] = 2
    hole_px = np.frombuffer(np.uint32(hole_rgba8).tobytes(), np.uint8)
    src = np.asarray(src_rgba, np.uint8).reshape(n, 4)
    colour = np.where((mask > 0)[:, None], src[np.maximum(take, 0)], hole_px[None, :]).astype(np.uint8)
    depth = np.where(mask > 0, zc_of_src[np.maximum(take, 0)], 0).astype(F32)
    return colour, depth, mask, int(np.count_nonzero(mask == 0))


def reproject_f32(scene, w, h, camera_origin, src_rgba, depth, acc, src_pos, src_rot, dst_pos, dst_rot, acc_min=ACC_MIN, hole_rgba8=HOLE,
                  flags=FILL):
    """The definition.  Returns (colour uint8 [n,4], depth float32 [n], mask uint8 [n], holes, winner int64 [n]: the source pixel whose
    splat won the destination pixel, -1 for none)."""
    n = w * h
    ok, pix, zc, near = splat(scene, w, h, camera_origin, depth, acc, src_pos, src_rot, dst_pos, dst_rot, acc_min, F32)
    bits = np.where(near, zc.view(np.uint32), np.uint32(FAR_BITS)).astype(np.uint64)
    key = (bits << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    zbuf = np.full(n, EMPTY, np.uint64)
    np.minimum.at(zbuf, pix[ok], key[ok])      # the atomicMin: independent of the order
    winner = np.where(zbuf != EMPTY, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    rank = np.where(zbuf != EMPTY, zbuf, np.uint64(0))
    return _resolve(w, h, winner, rank, zc, src_rgba, hole_rgba8, flags & FILL) + (winner,)


def reproject_f64(scene, w, h, camera_origin, src_rgba, depth, acc, src_pos, src_rot, dst_pos, dst_rot, acc_min=ACC_MIN, hole_rgba8=HOLE,
                  flags=FILL):
    """The same geometry in float64: nearest camera depth wins, the lower source index on a tie; the fill takes the neighbour whose
    winner is farthest (higher index on a tie).  Same return as reproject_f32."""
    n = w * h
    ok, pix, zc, near = splat(scene, w, h, camera_origin, depth, acc, src_pos, src_rot, dst_pos, dst_rot, acc_min, np.float64)
    idx = np.flatnonzero(ok)
    order = idx[np.lexsort((idx, zc[idx], pix[idx]))]      # by pixel, then depth, then index
    first = np.ones(order.size, bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    winner = np.full(n, -1, np.int64)
    winner[pix[order[first]]] = order[first]
    won = np.flatnonzero(winner >= 0)
    by_depth = won[np.lexsort((winner[won], zc[winner[won]]))]
    rank = np.zeros(n, np.uint64)
    rank[by_depth] = np.arange(1, by_depth.size + 1, dtype=np.uint64)
    return _resolve(w, h, winner, rank, zc, src_rgba, hole_rgba8, flags & FILL) + (winner,)


# ---- the inputs of the tests -------------------------------------------------------------------------

SIZES = [(97, 61), (16, 12), (64, 1), (1, 1)]      # odd and ragged against 256-thread blocks; small; one row; one pixel
SRC_YAW, SRC_PITCH = 100.0, -5.0


def box_of(w, h):
    """the nearer box: the central third of the frame (x0, x1, y0, y1), empty for a frame too small"""
    return w // 3, w - w // 3, h // 4, h - h // 4


def depth_scene(w, h, seed, planted=True):
    """A wall at ~4 with a nearer box at ~1.5 in front of it (distances along the ray from its origin, smoothly varying so that depth
    ties are rare), acc in [0.8, 1]; planted: acc below ACC_MIN, acc = 0, NaN / inf / negative depth at scattered pixels and one whole
    row far.  Returns (rgba uint8 [h,w,4] random bytes, depth_map float32 [h*w], acc_map float32 [h*w], is_box bool [h*w])."""
    rng = np.random.default_rng(seed + 7919 * w + h)
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    row, col = np.divmod(np.arange(w * h), w)
    t = 4.0 + 0.30 * np.sin(0.37 * col + 0.5) + 0.20 * np.cos(0.23 * row)
    x0, x1, y0, y1 = box_of(w, h)
    is_box = (col >= x0) & (col < x1) & (row >= y0) & (row < y1) & (w >= 6) & (h >= 4)
    t = np.where(is_box, 1.5 + 0.05 * np.sin(0.41 * col) + 0.04 * np.cos(0.31 * row + 1.0), t)
    acc = (0.8 + 0.2 * rng.random(w * h)).astype(F32)
    depth = (t.astype(F32) * acc).astype(F32)      # depth_map = sum w z, acc_map = sum w
    if planted and w * h >= 12:
        k = rng.permutation(w * h)[:max(6, (w * h) // 16)]
        for j, i in enumerate(k):
            kind = j % 6
            if kind == 0:
                acc[i], depth[i] = F32(0.3), F32(0.3 * t[i])      # a surface, but below acc_min
            elif kind == 1:
                acc[i], depth[i] = F32(0), F32(0)                 # 0 / 0
            elif kind == 2:
                depth[i] = F32(np.nan)
            elif kind == 3:
                depth[i] = F32(np.inf)
            elif kind == 4:
                depth[i] = -depth[i]
            else:
                acc[i] = F32(np.nan)
        if h >= 3:
            acc[(h - 2) * w:(h - 1) * w] = F32(0.1)               # one whole row far
    return rgba, depth, acc, is_box


def src_pose(scene):
    return np.asarray(scene.view_cell_center, F32), O.camera_rotation(SRC_YAW, SRC_PITCH)


def moved(scene, right=0.0, up=0.0, forward=0.0, yaw=0.0):
    """the source pose moved along its own axes (world units) and turned about the world's z (degrees)"""
    pos, rot = src_pose(scene)
    rot = rot.astype(np.float64)
    p = pos.astype(np.float64) + right * rot[:, 0] + up * rot[:, 1] - forward * rot[:, 2]
    return p.astype(F32), O.camera_rotation(SRC_YAW + yaw, SRC_PITCH)


# name -> the destination pose's offsets from the source pose: the geometric cases of tests/test_gpu_reproject.py
MOTIONS = {
    "identity": dict(),
    "lateral": dict(right=0.1, up=0.03),
    "forward": dict(forward=0.3),                  # magnifies: cracks, and the fill
    "backward": dict(forward=-0.3),                # minifies: collisions
    "yaw20": dict(yaw=20.0),
    "behind_part": dict(forward=2.0),              # in front of the wall, behind the box: zc <= 0 for part of the scene
    "sees_none": dict(yaw=180.0),                  # every pixel a hole
}
