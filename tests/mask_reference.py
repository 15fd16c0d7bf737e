"""The definition adanerf_render_masked is tested against, in numpy (include/adanerf_hip.h): which pixels a byte mask selects, and what the
outputs of a masked render hold afterwards."""
import numpy as np


def selected(mask, values):
    """bool [n]: pixel p is rendered iff mask[p] < 32 and bit mask[p] of `values` is set"""
    m = np.asarray(mask, dtype=np.uint8).astype(np.uint64)
    bits = (np.uint64(int(values) & 0xFFFFFFFF) >> np.minimum(m, np.uint64(31))) & np.uint64(1)
    return (m < 32) & (bits == 1)


def list_of(mask, values):
    """int32 [M]: the ascending ids of the selected pixels"""
    return np.flatnonzero(selected(mask, values)).astype(np.int32)


def expected(before, full, mask, values):
    """the output after the call: the full frame's element where the pixel is selected, else what was there.  `before` / `full`: [n] or
    [n, k] arrays of one dtype."""
    before, full = np.asarray(before), np.asarray(full)
    assert before.shape == full.shape and before.dtype == full.dtype
    sel = selected(mask, values)
    return np.where(sel.reshape((-1,) + (1,) * (full.ndim - 1)), full, before)


# ---- the masks of the GPU tests (tests/test_gpu_render_masked.py), by name: (n, width) -> (mask uint8 [n], values) -------------------

def m_edges(which):
    def make(n, w):
        m = np.ones(n, np.uint8)
        if which == "first":
            m[0] = 0
        elif which == "last":
            m[n - 1] = 0
        elif which == "all":
            m[:] = 0
        elif which == "none":
            pass
        else:      # M = int(which): that many pixels spread over the frame by a fixed stride walk
            idx = (np.arange(int(which), dtype=np.int64) * 7919) % n
            assert len(np.unique(idx)) == int(which)
            m[idx] = 0
        return m, 1
    return make


def checkerboard(n, w):
    p = np.arange(n)
    return (((p % w) + (p // w)) & 1).astype(np.uint8), 1


def empty_segment(n, w):
    """one whole 32-ray segment without a selected pixel between full ones"""
    m = np.zeros(n, np.uint8)
    m[64:96] = 1
    return m, 1


def empty_tile(n, w):
    """a whole 128-ray tile without a selected pixel between full ones"""
    m = np.zeros(n, np.uint8)
    m[128:256] = 1
    return m, 1


def random30(n, w):
    rng = np.random.default_rng(20240607)
    return (rng.random(n) >= 0.3).astype(np.uint8), 1


def mixed_bytes(n, w):
    """the bytes 0, 1, 2, 31, 32, 255 with values 5: 0 and 2 select"""
    rng = np.random.default_rng(77)
    return rng.choice(np.array([0, 1, 2, 31, 32, 255], np.uint8), size=n), 5


MASKS = {"m1_first": m_edges("first"), "m1_last": m_edges("last"), "m127": m_edges(127), "m128": m_edges(128), "m129": m_edges(129), "all": m_edges("all"),
         "checkerboard": checkerboard, "empty_segment": empty_segment, "empty_tile": empty_tile, "random30": random30, "mixed_bytes": mixed_bytes}
