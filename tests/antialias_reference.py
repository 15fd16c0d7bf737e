"""Restatements of the anti-aliasing entry points (include/adanerf_hip.h: adanerf_set_pixel_offset, adanerf_host_subpixel_grid,
adanerf_accumulate / adanerf_resolve_mean, ADANERF_PRESENT_AREA) -- held apart from the library, so that the reference is never the
code under test.  Everything here is exact: the GPU tests ask for equality.

  area_present     the area filter in numpy integers (int64), from the definition's overlap weights
  accumulate_f32 / resolve_f32   numpy float32: every numpy float32 array operation is one rounded fp32 operation, which is what the
                   kernels' __fadd_rn and IEEE division are; the 8-bit image is the viewer's output contract
  ray_table / rays the float64 ray table built from start + pp * col, so that the offset can enter as the header defines it
                   (start' = start + pp * (double)dx: a rounded multiply, then a rounded add), over tests/reproject_reference.py's
                   float32 gen_ray.  At offset (0, 0) it is oracle.generate_ray_directions bit for bit (tests/test_antialias_cpu.py)."""
import numpy as np

import adanerf_oracle as O
import reproject_reference as RR

F32 = np.float32
AREA = 8                       # ADANERF_PRESENT_AREA
AREA_MAX_RATIO = 8
# (src_w, src_h, dst_w, dst_h): identity, exact 2 x, odd and ragged against 256-thread blocks, one row, 8 x, enlarging, ratio 7.9 on one row
AREA_SIZES = [(7, 5, 7, 5), (8, 6, 4, 3), (97, 61, 41, 23), (64, 1, 9, 1), (16, 16, 2, 2), (5, 5, 8, 8), (300, 3, 38, 1)]
# the sizes the definition's properties were stated at (CPU)
AREA_PROPERTY_SIZES = [(7, 5, 7, 5), (8, 6, 4, 3), (97, 61, 41, 23), (64, 1, 9, 1), (16, 16, 2, 2), (5, 5, 8, 8), (9, 7, 2, 1), (33, 17, 5, 3)]
OFFSETS = [(0.0, 0.0), (0.25, -0.25), (-0.5, 0.5), (1.0, -1.0)]
RAY_SIZES = [(97, 61), (16, 12), (1, 1)]


# ---- the sub-pixel grid ------------------------------------------------------------------------------

def subpixel_grid(s):
    """[(dx, dy)] for k in 0..s*s-1: i = k % s, j = k / s, dx = (2 i + 1 - s) / (2 s) in double, cast to float"""
    return [(float(F32((2.0 * (k % s) + 1.0 - s) / (2.0 * s))), float(F32((2.0 * (k // s) + 1.0 - s) / (2.0 * s)))) for k in range(s * s)]


# ---- the area filter ---------------------------------------------------------------------------------

def area_weights(src, dst):
    """[dst, src] int64: overlap of destination pixel x = [x src, (x + 1) src) with source pixel i = [i dst, (i + 1) dst)"""
    x = np.arange(dst, dtype=np.int64)[:, None]
    i = np.arange(src, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * dst, (x + 1) * src) - np.maximum(i * dst, x * src))


def area_taps(src, dst):
    """first and last contributing source pixel of every destination pixel"""
    x = np.arange(dst, dtype=np.int64)
    return (x * src) // dst, ((x + 1) * src - 1) // dst


def area_present(img, dst_w, dst_h, flip_y=False):
    """img uint8 [src_h, src_w, 4] -> uint8 [dst_h, dst_w, 4]: out = floor((2 V + S) / (2 S)), V = sum wy wx v, S = src_w src_h"""
    img = np.asarray(img, np.uint8)
    src_h, src_w = img.shape[:2]
    wx, wy = area_weights(src_w, dst_w), area_weights(src_h, dst_h)
    v = np.einsum("yj,xi,jic->yxc", wy, wx, img.astype(np.int64))
    s = np.int64(src_w) * np.int64(src_h)
    out = (2 * v + s) // (2 * s)
    assert out.min() >= 0 and out.max() <= 255
    out = out.astype(np.uint8)
    return out[::-1].copy() if flip_y else out


# ---- accumulate / resolve ----------------------------------------------------------------------------

def accumulate_f32(total, rgb, first):
    """sum = rgb (first) or sum + rgb, float32"""
    rgb = np.asarray(rgb, F32)
    if first:
        return rgb.copy()
    with np.errstate(all="ignore"):
        out = np.asarray(total, F32) + rgb
    assert out.dtype == F32
    return out


def rgba8_of(rgb):
    """the viewer's output contract, as the compositing kernels write it: (uchar)(fminf(fmaxf(v, 0), 1) * 255.0f), A = 255; fmaxf of a
    NaN and 0 is 0"""
    rgb = np.asarray(rgb, F32)
    with np.errstate(all="ignore"):
        c = np.where(np.isnan(rgb), F32(0), np.minimum(np.maximum(rgb, F32(0)), F32(1))) * F32(255.0)
    assert c.dtype == F32
    out = np.full(rgb.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = np.trunc(c).astype(np.uint8)
    return out


def resolve_f32(total, frames):
    """(mean float32 [n,3], rgba8 uint8 [n,4]): mean = sum / float32(frames), one IEEE division"""
    with np.errstate(all="ignore"):
        m = np.asarray(total, F32) / F32(frames)
    assert m.dtype == F32
    return m, rgba8_of(m)


# ---- the ray table with an offset ----------------------------------------------------------------------

def ray_table(w, h, fov, dx=0.0, dy=0.0):
    """Camera-space unit directions [h*w, 3] float32 of src/util/raygeneration.py:10-26 with the ray of pixel (x, y) through
    (x + 0.5 + dx, y + 0.5 + dy): float64 arithmetic, start' = start + pp * float64(float32(d)) -- two rounded operations, and not at all
    for a component equal to 0 -- then start' + pp * col as the kernels' gen_ray computes it."""
    focal = O.focal_from_fov(w, fov)
    x_dist = np.tan(fov / 2) * focal
    y_dist = x_dist * (h / w)
    x_pp = np.float64(x_dist / (w / 2))
    y_pp = np.float64(y_dist / (h / 2))
    start_x, start_y = np.float64(-(x_dist - x_pp / 2)), np.float64(-(y_dist - y_pp / 2))
    dx, dy = np.float64(F32(dx)), np.float64(F32(dy))
    if dx != 0:
        m = x_pp * dx
        start_x = start_x + m
    if dy != 0:
        m = y_pp * dy
        start_y = start_y + m
    col = np.arange(w, dtype=np.float64)[None, :].repeat(h, 0)
    row = np.arange(h, dtype=np.float64)[:, None].repeat(w, 1)
    v = np.empty((h, w, 3), dtype=np.float64)
    v[..., 0] = start_x + x_pp * col
    v[..., 1] = start_y + y_pp * row
    v[..., 2] = focal
    v /= np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])[..., None]
    v[..., 1] *= -1.0
    v[..., 2] *= -1.0
    return v.reshape(h * w, 3).astype(F32)


def local_pixels(w, h, strip_rows=8, world=1, rank=0):
    """row-major pixel index of every local ray of `rank` under round-robin row strips (k_common.hip.hpp ray_pixel)"""
    rows = [r for r in range(h) if (r // strip_rows) % world == rank]
    return (np.asarray(rows, np.int64)[:, None] * w + np.arange(w, dtype=np.int64)[None, :]).reshape(-1)


def rays(scene, w, h, pos, rot, dx=0.0, dy=0.0, camera_origin=False, strip_rows=8, world=1, rank=0):
    """[n_local, 8] float32 as ADANERF_BUF_RAYS / d_rays_out hold them: (origin.xyz, 0, direction.xyz, 0); origin = the view-cell sphere
    exit, or the camera position (coarse/fine models).  tests/reproject_reference.py rays_f32 over the offset table."""
    d = ray_table(w, h, scene.fov, dx, dy)
    rot = np.asarray(rot, F32).reshape(9)
    pos = np.asarray(pos, F32).reshape(3)
    nds = np.stack([(rot[3 * i] * d[:, 0] + rot[3 * i + 1] * d[:, 1]) + rot[3 * i + 2] * d[:, 2] for i in range(3)], axis=1)
    c = np.asarray(scene.view_cell_center, F32)
    q = pos - c
    udot = (q[0] * nds[:, 0] + q[1] * nds[:, 1]) + q[2] * nds[:, 2]
    qq = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
    delta = udot * udot - (qq - F32(RR._rad2(scene)))
    dist = -udot + np.sqrt(np.maximum(delta, F32(0)))
    p = pos[None, :] + nds * dist[:, None]
    assert nds.dtype == F32 and p.dtype == F32
    out = np.zeros((w * h, 8), F32)
    out[:, 0:3] = np.broadcast_to(pos[None, :], p.shape) if camera_origin else p
    out[:, 4:7] = nds
    return out[local_pixels(w, h, strip_rows, world, rank)]
