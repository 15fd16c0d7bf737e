"""numpy float32 restatements of adaptive supersampling's three device calls, as include/adanerf_hip.h defines them.

contrast_mask             adanerf_contrast_mask / adanerf_host_contrast_mask by brute force: an explicit loop over the 8 neighbour offsets, each
                          applied to every pixel that has such a neighbour inside the image; every difference one np.float32 subtraction.
accumulate_masked         adanerf_accumulate_masked: one np.float32 addition per value of a selected pixel; the rest is copied by its bits.
resolve_mean_masked       adanerf_resolve_mean_masked: one np.float32 division per value of a selected pixel, the viewer's byte contract
                          (antialias_reference.rgba8_of) for the 8-bit image; the rest is copied by its bits.
faulty_masks              the same mask under rules that are wrong in one way each -- what the tests show the reference rejects.
"""
import numpy as np

import antialias_reference as AR

f32 = np.float32


def display(rgb):
    """v = fminf(fmaxf(x, 0), 1): a NaN is 0, -inf 0, +inf 1 (np.fmax / np.fmin return the other operand for a NaN, as fmaxf / fminf do)"""
    a = np.asarray(rgb, dtype=f32)
    return np.fmin(np.fmax(a, f32(0)), f32(1)).astype(f32)


def contrast_mask(rgb, w, h, threshold, neighbours=None, strict=True, clamp=True):
    """(mask [h*w] uint8, n_flagged).  The keyword arguments exist for faulty_masks only."""
    v = display(rgb) if clamp else np.asarray(rgb, dtype=f32)
    v = v.reshape(h, w, 3)
    thr = f32(threshold)
    if neighbours is None:
        neighbours = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
    flagged = np.zeros((h, w), dtype=bool)
    with np.errstate(invalid="ignore"):
        for dx, dy in neighbours:      # one neighbour at a time, over the pixels p for which q = p + (dx, dy) lies inside the image
            x0, x1, y0, y1 = max(0, -dx), min(w, w - dx), max(0, -dy), min(h, h - dy)
            if x0 >= x1 or y0 >= y1:
                continue
            p = v[y0:y1, x0:x1]
            q = v[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            d = np.abs(p - q)      # float32 arrays: one rounded fp32 subtraction per value
            assert d.dtype == f32
            c = np.maximum(np.maximum(d[..., 0], d[..., 1]), d[..., 2])      # no NaN unless the clamp is off, where a NaN flags nothing
            flagged[y0:y1, x0:x1] |= (c > thr) if strict else (c >= thr)
    mask = np.where(flagged, 0, 1).astype(np.uint8).reshape(-1)
    return mask, int(np.count_nonzero(mask == 0))


def faulty_masks(rgb, w, h, threshold):
    """{name: mask} of three rules that are each wrong in one way"""
    return {
        "no diagonals": contrast_mask(rgb, w, h, threshold, neighbours=[(-1, 0), (1, 0), (0, -1), (0, 1)])[0],
        ">= instead of >": contrast_mask(rgb, w, h, threshold, strict=False)[0],
        "no clamp": contrast_mask(rgb, w, h, threshold, clamp=False)[0],
    }


def selected(mask, values):
    """adanerf_render_masked's selection: mask[p] < 32 and bit mask[p] of values set"""
    m = np.asarray(mask, dtype=np.uint8).astype(np.int64)
    return (m < 32) & (((int(values) & 0xFFFFFFFF) >> np.minimum(m, 31)) & 1).astype(bool)


def accumulate_masked(rgb, mask, values, sum_in, first):
    """the new sum [n,3] fp32: selected pixels rgb (first) or sum + rgb, the others the bits of sum_in"""
    rgb = np.asarray(rgb, dtype=f32).reshape(-1, 3)
    out = np.array(sum_in, dtype=f32).reshape(-1, 3).copy()
    sel = selected(mask, values)
    with np.errstate(invalid="ignore", over="ignore"):
        new = rgb[sel] if first else (out[sel] + rgb[sel]).astype(f32)
    out.view(np.uint32)[sel] = np.ascontiguousarray(new).view(np.uint32)
    return out


def resolve_mean_masked(sum_in, mask, values, frames, rgb_before, rgba8_before):
    """(rgb [n,3] fp32, rgba8 [n,4] uint8): selected pixels sum / frames and its bytes, the others the bits of the images before"""
    s = np.asarray(sum_in, dtype=f32).reshape(-1, 3)
    rgb = np.array(rgb_before, dtype=f32).reshape(-1, 3).copy()
    rgba = np.array(rgba8_before, dtype=np.uint8).reshape(-1, 4).copy()
    sel = selected(mask, values)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = (s[sel] / f32(frames)).astype(f32)
    rgb.view(np.uint32)[sel] = np.ascontiguousarray(m).view(np.uint32)
    rgba[sel] = AR.rgba8_of(m)
    return rgb, rgba
