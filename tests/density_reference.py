"""Restatements of the foveated ray density entry points (include/adanerf_hip.h: adanerf_foveate_density / adanerf_host_density_mask,
adanerf_fill_density) in numpy.  The mask follows the header's definition by brute force -- the smallest stride over every pixel of the
box, not the closed form the library uses for the pixel nearest the gaze -- and the fill does every step as one float32 operation in
the header's order.  Nothing here calls the library."""
import numpy as np

LEVELS = (1, 2, 4, 8)


def half_px(g):
    """lrintf(2 g) clamped to +-2^31: round half to even, as adanerf_foveate does it"""
    v = np.float32(2.0) * np.float32(g)
    v = min(max(float(v), -2147483648.0), 2147483648.0)
    return int(np.rint(v))


def stride_map(w, h, gaze, radius_px, stride):
    """s(x, y) [h, w] int64: the stride of the first ring that contains the pixel, the last entry outside them all"""
    gx2, gy2 = half_px(gaze[0]), half_px(gaze[1])
    x = np.arange(w, dtype=object)[None, :]      # Python integers: q passes 2^63 for a gaze at the clamp
    y = np.arange(h, dtype=object)[:, None]
    q = (2 * x + 1 - gx2) ** 2 + (2 * y + 1 - gy2) ** 2
    s = np.full((h, w), int(stride[len(radius_px)]), dtype=np.int64)
    for k in reversed(range(len(radius_px))):
        inside = (q <= 4 * int(radius_px[k]) ** 2).astype(bool)
        s[inside] = int(stride[k])
    return s


def density_mask(w, h, gaze, radius_px, stride):
    """[h*w] uint8: 0 where some level L divides x and y and the box of L - 1 pixels around the pixel (clipped) holds a stride <= L; the
    pixel's own stride elsewhere"""
    s = stride_map(w, h, gaze, radius_px, stride)
    out = s.astype(np.uint8)
    for y in range(h):
        for x in range(w):
            for L in LEVELS:
                if x % L or y % L:
                    continue
                box = s[max(y - L + 1, 0):min(y + L - 1, h - 1) + 1, max(x - L + 1, 0):min(x + L - 1, w - 1) + 1]
                if box.min() <= L:
                    out[y, x] = 0
                    break
    return out.reshape(-1)


def corners(x, y, s, w, h):
    """(x0, x1, y0, y1) of a pixel with mask byte s"""
    x0, y0 = x & ~(s - 1), y & ~(s - 1)
    x1 = x0 if (x == x0 or x0 + s >= w) else x0 + s
    y1 = y0 if (y == y0 or y0 + s >= h) else y0 + s
    return x0, x1, y0, y1


def used_corners(x, y, s, w, h):
    """the distinct corner pixels as flat indices"""
    x0, x1, y0, y1 = corners(x, y, s, w, h)
    return sorted({yy * w + xx for yy in (y0, y1) for xx in (x0, x1)})


def _lerp(a, b, f):
    """a + f (b - a), three rounded float32 operations; a, b arrays of one dtype float32"""
    with np.errstate(all="ignore"):
        d = (b - a).astype(np.float32)
        p = (np.float32(f) * d).astype(np.float32)
        return (a + p).astype(np.float32)


def _blend(img, w, x, y, s, x0, x1, y0, y1):
    c00, c01, c10, c11 = img[y0 * w + x0], img[y0 * w + x1], img[y1 * w + x0], img[y1 * w + x1]
    fx = np.float32(x - x0) / np.float32(s)
    fy = np.float32(y - y0) / np.float32(s)
    top = c00 if x1 == x0 else _lerp(c00, c01, fx)
    if y1 == y0:
        return top
    bot = c10 if x1 == x0 else _lerp(c10, c11, fx)
    return _lerp(top, bot, fy)


def rgba8_of(rgb):
    """adanerf_resolve_mean's byte contract: (uchar)(clamp(v, 0, 1) * 255), a NaN gives 0, A = 255; rgb [3] float32"""
    with np.errstate(all="ignore"):
        v = np.where(np.isnan(rgb), np.float32(0), np.minimum(np.maximum(rgb, np.float32(0)), np.float32(1))).astype(np.float32)
        b = (v * np.float32(255)).astype(np.float32).astype(np.uint8)
    return np.array([b[0], b[1], b[2], 255], np.uint8)


def fill(mask, w, h, rgb, depth=None, acc=None, rgba8=None):
    """(rgb, depth, acc, rgba8, unfilled) after adanerf_fill_density: copies of the inputs ([h*w,3] / [h*w] float32, [h*w,4] uint8, None
    stays None) with every pixel of byte 2, 4 or 8 whose used corners all carry byte 0 replaced"""
    mask = np.asarray(mask, np.uint8).reshape(-1)
    src = [np.asarray(rgb, np.float32).reshape(h * w, 3), None if depth is None else np.asarray(depth, np.float32).reshape(-1),
           None if acc is None else np.asarray(acc, np.float32).reshape(-1)]
    out = [None if a is None else a.copy() for a in src]
    out8 = None if rgba8 is None else np.asarray(rgba8, np.uint8).reshape(h * w, 4).copy()
    unfilled = 0
    for p in np.flatnonzero((mask == 2) | (mask == 4) | (mask == 8)).tolist():
        s = int(mask[p])
        y, x = divmod(p, w)
        if any(mask[c] != 0 for c in used_corners(x, y, s, w, h)):
            unfilled += 1
            continue
        x0, x1, y0, y1 = corners(x, y, s, w, h)
        for a, o in zip(src, out):
            if a is not None:
                o[p] = _blend(a, w, x, y, s, x0, x1, y0, y1)      # corners carry byte 0: never rewritten, src == out there
        if out8 is not None:
            out8[p] = rgba8_of(out[0][p])
    return out[0], out[1], out[2], out8, unfilled


def parse_spec(spec):
    """'R:S[,R:S...],S' -> (radius_px list, stride list) without any checking: the tests' own reading of their settings"""
    parts = spec.split(",")
    rings = [p.split(":") for p in parts[:-1]]
    return [int(r[0]) for r in rings], [int(r[1]) for r in rings] + [int(parts[-1])]
