"""numpy restatement of hybrid rendering (adanerf_set_depth_limit / adanerf_compact_depth_limit / adanerf_blend_behind /
adanerf_host_sphere_zc): the camera-space depth of a selected bin in float32 arrays, one operation per statement; the trim of a selected
row; the blend; the sphere in float64.  numpy rounds every array operation once and fuses nothing, so everything that compares against
this file compares bytes.  Test infrastructure: nothing under adanerf_amd/ imports it."""
import numpy as np

from antialias_reference import rgba8_of

F32 = np.float32
F64 = np.float64


def sample_zc(rays, ztab, bins, pos, rot):
    """zc [R, N] float32 of every entry of a selection in select_adaptive's layout ([R, N] bins, -1 padded: those give the zc of bin 0,
    never looked at): z = ztab[b]; P_i = o_i + d_i z; q_i = P_i - pos_i; zc = -((R[2] q_0 + R[5] q_1) + R[8] q_2)."""
    rays = np.asarray(rays, F32).reshape(-1, 8)
    ztab, pos, rot = np.asarray(ztab, F32), np.asarray(pos, F32).reshape(3), np.asarray(rot, F32).reshape(9)
    b = np.maximum(np.asarray(bins).astype(np.int64), 0)
    z = ztab[b]
    q = []
    with np.errstate(all="ignore"):
        for i in range(3):
            m = rays[:, 4 + i, None] * z
            p = rays[:, i, None] + m
            q.append(p - pos[i])
        t0 = rot[2] * q[0]
        t1 = rot[5] * q[1]
        t2 = rot[8] * q[2]
        s = t0 + t1
        s = s + t2
        zc = -s
    assert zc.dtype == F32
    return zc


def trim(count, bins, wts, zc, limit):
    """The depth trim of a selection in select_adaptive's layout ([R] counts, [R, N] bins -1 padded, [R, N] values 0 padded): entry k of
    ray r is dropped iff zc[r, k] >= limit[r] (a NaN on either side keeps it); survivors keep their order and values.  Returns the same
    layout; counts may be 0."""
    count = np.asarray(count).astype(np.int32)
    limit = np.asarray(limit, F32)
    valid = np.arange(bins.shape[1])[None, :] < count[:, None]
    with np.errstate(invalid="ignore"):
        keep = valid & ~(zc >= limit[:, None])
    oc = keep.sum(axis=1).astype(np.int32)
    ob, ow = np.full_like(bins, -1), np.zeros_like(wts)
    dst = np.cumsum(keep, axis=1) - 1      # position of a survivor in its row
    rr, kk = np.nonzero(keep)
    ob[rr, dst[rr, kk]] = bins[rr, kk]
    ow[rr, dst[rr, kk]] = wts[rr, kk]
    return oc, ob, ow


def blend(rgb, acc, behind):
    """(out float32 [n,3], rgba8 uint8 [n,4]): t = 1 - acc; !(t > 0) -> 0; t > 1 -> 1; t == 0: out = rgb, the bits; else
    out_c = rgb_c + t * behind_c (a product, then a sum)"""
    rgb, behind = np.asarray(rgb, F32).reshape(-1, 3), np.asarray(behind, F32).reshape(-1, 3)
    acc = np.asarray(acc, F32).reshape(-1)
    with np.errstate(all="ignore"):
        t = F32(1.0) - acc
        t = np.where(t > F32(0), t, F32(0)).astype(F32)
        t = np.where(t > F32(1), F32(1), t).astype(F32)
        m = t[:, None] * behind
        s = rgb + m
    assert s.dtype == F32
    out = np.where((t == F32(0))[:, None], rgb, s)
    return out, rgba8_of(out)


def sphere(width, height, focal, pos, rot, center, radius):
    """(zc float32 [h*w], disc float64 [h*w]) of adanerf_host_sphere_zc, in float64, each step one rounded operation in the header's
    order; the inputs are float32 values as the C ABI receives them."""
    pos, center = np.asarray(pos, F32).astype(F64).reshape(3), np.asarray(center, F32).astype(F64).reshape(3)
    R = np.asarray(rot, F32).astype(F64).reshape(9)
    f, rad = F64(F32(focal)), F64(F32(radius))
    e = center - pos
    c = []
    for k in range(3):
        m0, m1, m2 = R[k] * e[0], R[3 + k] * e[1], R[6 + k] * e[2]
        s = m0 + m1
        c.append(s + m2)
    s = c[0] * c[0] + c[1] * c[1]
    cc = s + c[2] * c[2]
    g = cc - rad * rad
    x = np.arange(width, dtype=F64)[None, :]
    y = np.arange(height, dtype=F64)[:, None]
    vx = ((x + 0.5) - 0.5 * width) / f
    vy = -(((y + 0.5) - 0.5 * height) / f)
    s = vx * vx + vy * vy
    a = s + 1.0
    s = vx * c[0] + vy * c[1]
    b = s - c[2]
    disc = b * b - a * g
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = np.sqrt(np.where(disc >= 0, disc, 0.0))
        t0 = (b - q) / a
        t1 = (b + q) / a
        zc = np.where(disc >= 0, np.where(t0 > 0, t0, np.where(t1 > 0, t1, np.inf)), np.inf).astype(F32)
    return zc.reshape(-1), disc.reshape(-1)
