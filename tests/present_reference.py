"""The arithmetic of adanerf_present (include/adanerf_hip.h) restated in numpy int64: what the present kernel must reproduce bit for
bit.  Per axis, destination pixel x of d from a source of s pixels, D = 2 d:  n = (2 x + 1) s - d,  i0 = floor(n / D),  f = n - i0 D;
taps clamp(i0), clamp(i0 + 1) with weights D - f, f.  Per channel v = the four weighted taps, out = floor((2 v + D E) / (2 D E)).
Nearest: i = min(floor((2 x + 1) s / D), s - 1).  Filter rule (the viewer's blit): linear if dst_w > src_w, else nearest."""
import numpy as np

FLIP_Y, NEAREST, LINEAR = 1, 2, 4
MAX_SIDE = 16384


def linear_taps(s: int, d: int):
    """(t0, t1, f) int64 [d]: the two clamped taps of every destination pixel of one axis and the weight of the second."""
    x = np.arange(d, dtype=np.int64)
    D = 2 * d
    n = (2 * x + 1) * s - d
    i0 = n // D                     # numpy's // floors, also below zero
    f = n - i0 * D
    return np.clip(i0, 0, s - 1), np.clip(i0 + 1, 0, s - 1), f


def nearest_taps(s: int, d: int):
    x = np.arange(d, dtype=np.int64)
    return np.minimum(((2 * x + 1) * s) // (2 * d), s - 1)


def uses_linear(src_w: int, dst_w: int, flags: int = 0) -> bool:
    if flags & NEAREST and flags & LINEAR:
        raise ValueError("both filters")
    if flags & (NEAREST | LINEAR):
        return bool(flags & LINEAR)
    return dst_w > src_w


def present(src: np.ndarray, dst_w: int, dst_h: int, flags: int = 0) -> np.ndarray:
    """src uint8 [src_h, src_w, 4] -> uint8 [dst_h, dst_w, 4]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 4
    sh, sw = src.shape[:2]
    assert 1 <= min(sw, sh, dst_w, dst_h) and max(sw, sh, dst_w, dst_h) <= MAX_SIDE
    if uses_linear(sw, dst_w, flags):
        xa, xb, fx = linear_taps(sw, dst_w)
        ya, yb, fy = linear_taps(sh, dst_h)
        D, E = 2 * dst_w, 2 * dst_h
        p = src.astype(np.int64)
        wx0, wx1 = (D - fx)[None, :, None], fx[None, :, None]
        wy0, wy1 = (E - fy)[:, None, None], fy[:, None, None]
        top = wx0 * p[ya][:, xa] + wx1 * p[ya][:, xb]
        bot = wx0 * p[yb][:, xa] + wx1 * p[yb][:, xb]
        v = wy0 * top + wy1 * bot
        out = ((2 * v + D * E) // (2 * D * E)).astype(np.uint8)
    else:
        out = src[nearest_taps(sh, dst_h)][:, nearest_taps(sw, dst_w)]
    return np.ascontiguousarray(out[::-1] if flags & FLIP_Y else out)


def tap_bounds(src: np.ndarray, dst_w: int, dst_h: int):
    """(min, max) uint8 [dst_h, dst_w, 4] over the four taps of the linear filter (top-down order)."""
    sh, sw = src.shape[:2]
    xa, xb, _ = linear_taps(sw, dst_w)
    ya, yb, _ = linear_taps(sh, dst_h)
    taps = np.stack([src[ya][:, xa], src[ya][:, xb], src[yb][:, xa], src[yb][:, xb]])
    return taps.min(axis=0), taps.max(axis=0)
