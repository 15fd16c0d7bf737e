"""Restatements of adanerf_reproject_pair (include/adanerf_hip.h) and the inputs its tests use -- held apart from the library, so that
the reference is never the code under test.

pair_f32 is the definition operation by operation in numpy float32 (every numpy float32 array operation is one rounded fp32 operation,
which is what the kernels' __fsub_rn / __fmul_rn / __fadd_rn are): per source the splat of tests/reproject_reference.py (splat and the
key it feeds the 64-bit minimum), then the resolve over the two z-buffers.  The GPU tests ask for equality with it.  pair_f64 is the same
geometry in float64: the tests' inputs must be such that the two agree on each source's winner and on the agree / disagree decision
nearly everywhere, which is a condition on the inputs, checked in tests/test_reproject_pair_cpu.py.

The rays, poses, sizes and the wall + box depth scene are those of tests/reproject_reference.py; the colours of the wall + box cases
those of tests/temporal_reference.py (NaNs and signed zeros planted, no infinities)."""
import collections

import numpy as np

import antialias_reference as AR
import reproject_reference as RR
from reproject_reference import ACC_MIN, EMPTY, FAR_BITS, FILL, HOLE, SIZES, depth_scene, moved, rays_f64, splat, src_pose      # noqa: F401
from temporal_reference import colours      # noqa: F401

F32 = np.float32
DEPTH_TOL = 0.05      # the hosts' default

Source = collections.namedtuple("Source", "rgb depth acc pos rot")      # one rendered frame: fp32 colour [n,3], depth_map, acc_map [n], its pose
Result = collections.namedtuple("Result", "rgb rgba8 depth mask source holes winner_a winner_b agree key_a key_b")


# ---- the z-buffer of one source ----------------------------------------------------------------------

def zbuffer_f32(scene, w, h, camera_origin, s, dst_pos, dst_rot, acc_min=ACC_MIN):
    """Z_s of the definition: [n] uint64, EMPTY where no source pixel lands -- adanerf_reproject's own (reproject_reference.reproject_f32
    builds the same array from the same splat)"""
    n = w * h
    ok, pix, zc, near = splat(scene, w, h, camera_origin, s.depth, s.acc, s.pos, s.rot, dst_pos, dst_rot, acc_min, F32)
    bits = np.where(near, zc.view(np.uint32), np.uint32(FAR_BITS)).astype(np.uint64)
    key = (bits << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    zbuf = np.full(n, EMPTY, np.uint64)
    np.minimum.at(zbuf, pix[ok], key[ok])      # the atomicMin: independent of the order
    return zbuf


def _winners_f64(scene, w, h, camera_origin, s, dst_pos, dst_rot, acc_min):
    """(winner [n] int64 or -1, z [n] float64 of the winner, +inf for a far one): nearest camera depth, the lower source index on a tie"""
    n = w * h
    ok, pix, zc, _ = splat(scene, w, h, camera_origin, s.depth, s.acc, s.pos, s.rot, dst_pos, dst_rot, acc_min, np.float64)
    idx = np.flatnonzero(ok)
    order = idx[np.lexsort((idx, zc[idx], pix[idx]))]      # by pixel, then depth, then index
    first = np.ones(order.size, bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    winner = np.full(n, -1, np.int64)
    winner[pix[order[first]]] = order[first]
    return winner, np.where(winner >= 0, zc[np.maximum(winner, 0)], np.inf)


# ---- resolve ---------------------------------------------------------------------------------------

def _farthest_neighbour(w, h, key):
    """[n] uint64: the largest key among each pixel's 8 neighbours, 0 for none (key: 0 where there is no winner)"""
    pad = np.zeros((h + 2, w + 2), np.uint64)
    pad[1:-1, 1:-1] = key.reshape(h, w)
    best = np.zeros((h, w), np.uint64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                best = np.maximum(best, pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
    return best.reshape(-1)


def _resolve(w, h, T, a, b, win, z, key, weight_b, depth_tol, hole_rgba8, fill):
    """win / z / key: per source [A, B] the winner's source index (-1: none), its camera depth in T (+inf: far) and a uint64 that orders
    the winners of BOTH sources as the definition's keys do (0: none).  Everything after the z-buffers, in T."""
    n = w * h
    has = [win[0] >= 0, win[1] >= 0]
    far = [np.isinf(z[0]), np.isinf(z[1])]
    wb, tol = T(F32(weight_b)), T(F32(depth_tol))
    with np.errstate(all="ignore"):
        close = np.abs(z[0] - z[1]) <= tol * np.minimum(z[0], z[1])
        both = has[0] & has[1]
        agree = both & ((far[0] & far[1]) | (~far[0] & ~far[1] & close))
        b_nearer = z[1] < z[0]      # the smaller high word: positive floats order as their bits, +inf above all
        source = np.where(agree, 3, np.where(both, np.where(b_nearer, 2, 1), np.where(has[0], 1, np.where(has[1], 2, 0)))).astype(np.uint8)
        mask = (source > 0).astype(np.uint8)
        take = [win[0].copy(), win[1].copy()]
        zt = [z[0].copy(), z[1].copy()]
        if fill:
            best = [_farthest_neighbour(w, h, key[0]), _farthest_neighbour(w, h, key[1])]
            filled = (source == 0) & ((best[0] | best[1]) != 0)
            from_b = best[1] > best[0]      # on equal keys A
            source = np.where(filled, np.where(from_b, 2, 1), source).astype(np.uint8)
            mask[filled] = 2
            for s in (0, 1):      # the winner that owns the key: keys are unique within one z-buffer
                order = np.argsort(key[s], kind="stable")
                at = order[np.searchsorted(key[s], best[s], sorter=order).clip(0, n - 1)]
                ok = filled & (best[s] != 0)
                take[s] = np.where(ok, win[s][at], take[s])
                zt[s] = np.where(ok, z[s][at], zt[s])
        ca = np.asarray(a.rgb, F32).reshape(n, 3).astype(T)[np.maximum(take[0], 0)]
        cb = np.asarray(b.rgb, F32).reshape(n, 3).astype(T)[np.maximum(take[1], 0)]
        blend = ca + wb * (cb - ca)
        zblend = np.where(far[0] & far[1], T(np.inf), zt[0] + wb * (zt[1] - zt[0]))
        assert blend.dtype == T and zblend.dtype == T
        src3 = source[:, None]
        rgb = np.where(src3 == 3, blend, np.where(src3 == 1, ca, np.where(src3 == 2, cb, T(0)))).astype(F32)
        depth = np.where(source == 3, zblend, np.where(source == 1, zt[0], np.where(source == 2, zt[1], T(0)))).astype(F32)
    hole_px = np.frombuffer(np.uint32(hole_rgba8).tobytes(), np.uint8)
    rgba8 = np.where((mask > 0)[:, None], AR.rgba8_of(rgb), hole_px[None, :]).astype(np.uint8)
    return Result(rgb, rgba8, depth, mask, source, int(np.count_nonzero(mask == 0)), win[0], win[1], agree, key[0], key[1])


def pair_f32(scene, w, h, camera_origin, a, b, dst_pos, dst_rot, weight_b=0.5, acc_min=ACC_MIN, depth_tol=DEPTH_TOL, hole_rgba8=HOLE, flags=FILL):
    """The definition.  a, b: Source.  Returns Result(rgb [n,3] float32, rgba8 [n,4] uint8, depth [n] float32, mask [n] uint8, source [n]
    uint8, holes, winner_a / winner_b [n] int64: the source pixel that won the destination pixel in Z_A / Z_B (-1: none), agree [n] bool,
    key_a / key_b [n] uint64: the z-buffers with 0 for an empty pixel)."""
    win, z, key = [], [], []
    for s in (a, b):
        zbuf = zbuffer_f32(scene, w, h, camera_origin, s, dst_pos, dst_rot, acc_min)
        empty = zbuf == EMPTY
        win.append(np.where(empty, -1, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)))
        z.append(np.where(empty, F32(0), (zbuf >> np.uint64(32)).astype(np.uint32).view(F32)))
        key.append(np.where(empty, np.uint64(0), zbuf))
    return _resolve(w, h, F32, a, b, win, z, key, weight_b, depth_tol, hole_rgba8, flags & FILL)


def pair_f64(scene, w, h, camera_origin, a, b, dst_pos, dst_rot, weight_b=0.5, acc_min=ACC_MIN, depth_tol=DEPTH_TOL, hole_rgba8=HOLE, flags=FILL):
    """The same geometry in float64 (the colours too; they come back rounded to float32).  The keys are ranks: (depth, source index)
    ordered over the winners of both sources, equal pairs sharing a rank.  Same return as pair_f32."""
    n = w * h
    win, z = [], []
    for s in (a, b):
        wi, zi = _winners_f64(scene, w, h, camera_origin, s, dst_pos, dst_rot, acc_min)
        win.append(wi)
        z.append(zi)
    pairs = np.concatenate([np.stack([z[s], win[s].astype(np.float64)], axis=1) for s in (0, 1)])
    _, rank = np.unique(pairs, axis=0, return_inverse=True)
    rank = (rank.reshape(-1) + 1).astype(np.uint64)
    key = [np.where(win[s] >= 0, rank[s * n:(s + 1) * n], np.uint64(0)) for s in (0, 1)]
    return _resolve(w, h, np.float64, a, b, win, z, key, weight_b, depth_tol, hole_rgba8, flags & FILL)


# ---- the inputs of the tests -------------------------------------------------------------------------

# name -> (A, B, destination): offsets of tests/reproject_reference.py moved() from its source pose
CONSISTENT = {
    "lateral": (dict(right=-0.15), dict(right=0.15), dict(right=0.05)),
    "forward": (dict(forward=-0.3), dict(forward=0.3), dict(forward=0.1)),
    "yaw": (dict(yaw=-10.0), dict(yaw=10.0), dict(yaw=3.0)),
}
# two unrelated wall + box frames at two poses.  B is also moved along and turned about the view axis: after a move across it alone the two
# frames, whose depth is one function of (column, row), would give equal camera depths in exact arithmetic -- ties float32 and float64 break apart
INDEPENDENT = (dict(), dict(right=0.1, up=0.03, forward=0.05, yaw=2.0), dict(right=0.04, forward=0.1))


def _hit_sphere(o, d, centre, radius, far_side):
    """float64 distance along the unit rays (o, d) to the sphere: the near or the far intersection, +inf for a miss or one behind"""
    oc = o - centre[None, :]
    bq = np.sum(oc * d, axis=1)
    disc = bq * bq - (np.sum(oc * oc, axis=1) - radius * radius)
    root = np.sqrt(np.maximum(disc, 0.0))
    t = -bq + root if far_side else -bq - root
    return np.where((disc >= 0) & (t > 0), t, np.inf)


def consistent_view(scene, w, h, camera_origin, pos, rot, seed=0):
    """One view of the analytic scene both frames of a consistent pair look at: a ball of radius 0.5 at c0 + 2.2 fwd in front of a
    curved wall, the far side of a sphere of radius 12 centred at c0 - 7 fwd + 1.3 right + (0.2, 0.4, 0.9) (c0, fwd, right: the source
    pose of tests/reproject_reference.py).  A flat wall parallel to the image plane would put its lattice on pixel boundaries, where
    float32 and float64 part.  Ray-cast in float64 from the rays' origins; depth_map = t * acc with acc in [0.8, 1]; the colour is a smooth
    function of the world point.  Returns Source."""
    c0, r0 = src_pose(scene)
    c0, r0 = c0.astype(np.float64), np.asarray(r0, np.float64).reshape(3, 3)
    right, fwd = r0[:, 0], -r0[:, 2]
    ball_c = c0 + 2.2 * fwd
    wall_c = c0 - 7.0 * fwd + 1.3 * right + np.array([0.2, 0.4, 0.9])
    nds, p = rays_f64(scene, w, h, pos, rot)
    o = np.broadcast_to(np.asarray(pos, np.float64).reshape(1, 3), nds.shape) if camera_origin else p
    t = np.minimum(_hit_sphere(o, nds, ball_c, 0.5, False), _hit_sphere(o, nds, wall_c, 12.0, True))
    assert np.all(np.isfinite(t)) and np.all(t > 0)
    P = o + nds * t[:, None]
    rgb = np.stack([0.5 + 0.4 * np.sin(1.3 * P[:, 0] + 0.7 * P[:, 1]), 0.5 + 0.4 * np.cos(0.9 * P[:, 1] - 1.1 * P[:, 2]),
                    0.5 + 0.4 * np.sin(0.8 * P[:, 2] + 0.5 * P[:, 0] + 1.0)], axis=1).astype(F32)
    rng = np.random.default_rng(seed + 7919 * w + h)
    acc = (0.8 + 0.2 * rng.random(w * h)).astype(F32)
    depth = (t.astype(F32) * acc).astype(F32)
    return Source(rgb, depth, acc, np.asarray(pos, F32), np.asarray(rot, F32))


_CASES = {}


def case(scene, w, h, camera_origin, name):
    """(A, B, dst_pos, dst_rot) of the case `name`: a key of CONSISTENT, or "independent".  Computed once, shared and never changed."""
    k = (id(scene), w, h, camera_origin, name)
    if k not in _CASES:
        if name == "independent":
            pa, pb, pd = (moved(scene, **m) for m in INDEPENDENT)
            srcs = []
            for seed, pose in ((1, pa), (2, pb)):
                _, dm, acc, _ = depth_scene(w, h, seed)
                srcs.append(Source(colours(w, h, seed), dm, acc, pose[0], pose[1]))
            a, b = srcs
        else:
            pa, pb, pd = (moved(scene, **m) for m in CONSISTENT[name])
            a = consistent_view(scene, w, h, camera_origin, pa[0], pa[1], 1)
            b = consistent_view(scene, w, h, camera_origin, pb[0], pb[1], 2)
        for s in (a, b):
            for x in s[:3]:
                x.setflags(write=False)
        _CASES[k] = (a, b, pd[0], pd[1], scene)      # the scene is kept alive: its id is the key
    return _CASES[k][:4]


CASE_NAMES = list(CONSISTENT) + ["independent"]
