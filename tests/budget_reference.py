"""numpy restatement of the per-ray sample budgets (adanerf_set_budget_map / adanerf_foveate / adanerf_compact_budget): the effective
(n_r, thr_r) of a ray, the trim of a selected row, the selection a ray must end up with, and the ring fill of a gaze.  Exact arithmetic
only (integers and float comparisons), so everything that compares against this file compares bytes.  Test infrastructure: nothing under
adanerf_amd/ imports it."""
import numpy as np

import adanerf_oracle as O

from adanerf_amd import sharding

F32 = np.float32


def effective(n_map, thr_map, n_rays, n_max, thr):
    """(n_r [R] int32, thr_r [R] float32): 0 or a value above N is N; a threshold that is not above the context's (a NaN too) is the
    context's.  Either map may be None."""
    n = np.full(n_rays, n_max, np.int32)
    if n_map is not None:
        m = np.asarray(n_map).astype(np.int32)
        n = np.where((m == 0) | (m > n_max), n_max, m).astype(np.int32)
    t = np.full(n_rays, F32(thr), F32)
    if thr_map is not None:
        tm = np.asarray(thr_map, F32)
        with np.errstate(invalid="ignore"):
            t = np.where(tm > F32(thr), tm, F32(thr)).astype(F32)
    return n, t


def trim_row(bins, wts, n_r, thr_r):
    """The trim of one selected row (bins ascending, their values): the first n_r entries of the order (value descending, bin ascending)
    whose value is >= thr_r; the first of that order if none is; a row of one entry stays.  Returns (bins, values), bins ascending."""
    bins, wts = np.asarray(bins), np.asarray(wts, F32)
    c = len(bins)
    if c <= 1:
        return bins.copy(), wts.copy()
    order = sorted(range(c), key=lambda k: (-float(wts[k]), k))      # rows of more than one entry hold no NaN: every value reached a threshold
    keep = [k for k in order[:n_r] if wts[k] >= F32(thr_r)]
    if not keep:
        keep = order[:1]
    keep.sort()
    return bins[keep], wts[keep]


def trim(count, bins, wts, n_eff, thr_eff):
    """trim_row over a whole selection in select_adaptive's layout ([R] counts, [R, N] bins -1 padded, [R, N] values 0 padded)."""
    count = np.asarray(count).astype(np.int32).copy()
    ob, ow = np.full_like(bins, -1), np.zeros_like(wts)
    for r in range(len(count)):
        b, w = trim_row(bins[r, :count[r]], wts[r, :count[r]], int(n_eff[r]), thr_eff[r])
        count[r] = len(b)
        ob[r, :len(b)], ow[r, :len(b)] = b, w
    return count, ob, ow


def expected_selection(orc, n_max, thr, n_map=None, thr_map=None):
    """What ray r must carry: select_adaptive(orc[r:r+1], n_r, thr_r), rays grouped by distinct (n_r, thr_r); the layout of
    select_adaptive at n_max columns."""
    R = orc.shape[0]
    n_eff, thr_eff = effective(n_map, thr_map, R, n_max, thr)
    count = np.zeros(R, np.int32)
    bins = np.full((R, n_max), -1, np.int16)
    wts = np.zeros((R, n_max), F32)
    keys = np.stack([n_eff.astype(np.int64), thr_eff.view(np.uint32).astype(np.int64)], axis=1)
    for n_r, t_bits in np.unique(keys, axis=0):
        idx = np.flatnonzero((keys[:, 0] == n_r) & (keys[:, 1] == t_bits))
        t = np.array([t_bits], np.int64).astype(np.uint32).view(F32)[0]
        c, b, w = O.select_adaptive(orc[idx], int(n_r), t)
        count[idx] = c
        bins[idx, :int(n_r)] = b
        wts[idx, :int(n_r)] = w
    return count, bins, wts


def compacted(count, bins, wts):
    """(offsets, keys, values, total) of adanerf_compact's outputs for a selection in select_adaptive's layout"""
    count = np.asarray(count, np.int32)
    off = (np.cumsum(count) - count).astype(np.int32)
    m = np.arange(bins.shape[1])[None, :] < count[:, None]
    ray = np.broadcast_to(np.arange(len(count), dtype=np.uint32)[:, None], bins.shape)
    key = ((ray[m] << np.uint32(7)) | bins[m].astype(np.uint32)).astype(np.uint32)
    return off, key, wts[m].astype(F32), int(count.sum())


def gaze_half_pixels(g):
    """lrintf(2 g) clamped to +-2^31: twice the gaze, to the nearest integer, ties to even"""
    v = min(max(F32(2.0) * F32(g), F32(-2147483648.0)), F32(2147483648.0))
    return int(np.rint(np.float64(v)))


def ring_fill(w, h, gaze_xy, rings, strip_rows=8, world=1, rank=0):
    """(n_map uint8, thr_map float32) of the local rays of `rank`: rings = [(R, N, T), ..., (N, T)] (renderer.parse_fovea's form);
    q = (2 x + 1 - gx2)^2 + (2 y + 1 - gy2)^2; ring k contains the pixel iff q <= 4 R_k^2; the first ring that contains it, else the
    last entry.  Python integers: no overflow anywhere."""
    px = sharding.local_to_pixel(w, h, strip_rows, world, rank)
    gx2, gy2 = gaze_half_pixels(gaze_xy[0]), gaze_half_pixels(gaze_xy[1])
    n_map = np.empty(len(px), np.uint8)
    thr_map = np.empty(len(px), F32)
    radii = [int(r[0]) for r in rings[:-1]]
    for i, p in enumerate(px):
        y, x = divmod(int(p), w)
        q = (2 * x + 1 - gx2) ** 2 + (2 * y + 1 - gy2) ** 2
        k = next((j for j, rad in enumerate(radii) if q <= 4 * rad * rad), len(radii))
        n_map[i], thr_map[i] = rings[k][-2], F32(rings[k][-1])
    return n_map, thr_map
