"""FLIP (Andersson et al., HPG 2020) as the reference's evaluation computes it (src/evaluate.py:120-145 over
src/util/flip_loss.py:61-105), restated in numpy float64: what ``adanerf_flip`` and the fixtures of tools/gen_flip_golden.py are
held against.  Test infrastructure, in the role of tests/stage_reference.py.

The PARAMETERS are the reference's, rounded where it rounds them: the filter tables go through fp32 (``torch.Tensor(g)``; the
feature filters are normalised in fp32 after that), the D65 matrix is the fp32 one.  The ARITHMETIC on them is float64 throughout:
the matrix inverse, the reference illuminant, cmax, every convolution and every colour transform.  So the distance of the
reference's fp32 map from this one is the rounding error of its own arithmetic (``ref_fp32_residual`` in the fixtures), and the
device -- the same fp32 work in another order -- is held to a multiple of it.

NaN handling follows torch: clamp and maximum keep a NaN (np.clip / np.maximum do too), a comparison with a NaN is false.
"""
import numpy as np

DEFAULT_PPD = 0.7 * (3840 / 0.7) * (np.pi / 180)      # flip_loss.py:52-55
QC, QF, PC, PT = 0.7, 0.5, 0.4, 0.95


def radii(ppd):
    """(colour, feature) filter radius: flip_loss.py:142-144 (the largest scale parameter is b1_by = 0.04) and :221-222"""
    return int(np.ceil(3 * np.sqrt(0.04 / (2 * np.pi ** 2)) * ppd)), int(np.ceil(3 * (0.5 * 0.082 * ppd)))


def spatial_filter_table(ppd, channel):
    """generate_spatial_filter (flip_loss.py:112-154), fp32 [2r+1, 2r+1]"""
    a1, b1, a2, b2 = {"A": (1, 0.0047, 0, 1e-5), "RG": (1, 0.0053, 0, 1e-5), "BY": (34.1, 0.04, 13.5, 0.025)}[channel]
    r = radii(ppd)[0]
    dx = 1.0 / ppd
    x, y = np.meshgrid(range(-r, r + 1), range(-r, r + 1))
    z = (x * dx) ** 2 + (y * dx) ** 2
    g = a1 * np.sqrt(np.pi / b1) * np.exp(-np.pi ** 2 * z / b1) + a2 * np.sqrt(np.pi / b2) * np.exp(-np.pi ** 2 * z / b2)
    return (g / np.sum(g)).astype(np.float32)


def feature_filter_table(ppd, kind):
    """feature_detection's x-direction filter (flip_loss.py:216-240), fp32 [2r+1, 2r+1]; the y direction is its transpose"""
    sd = 0.5 * 0.082 * ppd
    r = radii(ppd)[1]
    x, y = np.meshgrid(range(-r, r + 1), range(-r, r + 1))
    g = np.exp(-(x ** 2 + y ** 2) / (2 * sd * sd))
    gx = np.multiply(-x, g) if kind == "edge" else np.multiply(x ** 2 / (sd * sd) - 1, g)
    neg, pos = np.float32(-np.sum(gx[gx < 0])), np.float32(np.sum(gx[gx > 0]))
    g32 = gx.astype(np.float32)
    return np.where(g32 < 0, g32 / neg, g32 / pos).astype(np.float32)


def rgb2xyz_matrix():
    """flip_loss.py:264-275, as the fp32 tensor holds it, in float64"""
    a = [[10135552 / 24577794, 8788810 / 24577794, 4435075 / 24577794],
         [2613072 / 12288897, 8788810 / 12288897, 887015 / 12288897],
         [1425312 / 73733382, 8788810 / 73733382, 70074185 / 73733382]]
    return np.array(a, np.float32).astype(np.float64)


A = rgb2xyz_matrix()
A_INV = np.linalg.inv(A)
ILLUM = A @ np.ones(3)


def srgb_to_ycxcz(img):
    """[..., 3] sRGB -> YCxCz ('srgb2ycxcz', flip_loss.py:250-254, 261-289)"""
    c = np.clip(np.asarray(img, np.float64), 0.0, 1.0)
    with np.errstate(invalid="ignore"):
        lin = np.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92)
    n = (lin @ A.T) / ILLUM
    return np.stack([116 * n[..., 1] - 16, 500 * (n[..., 0] - n[..., 1]), 200 * (n[..., 1] - n[..., 2])], axis=-1)


def linrgb_to_hunt_lab(rgb):
    """'linrgb2lab' (flip_loss.py:303-315) followed by hunt_adjustment (:181-193)"""
    n = (rgb @ A.T) / ILLUM
    delta = 6 / 29
    with np.errstate(invalid="ignore"):
        f = np.where(n > 0.00885, np.abs(n) ** (1 / 3), n / (3 * delta * delta) + 4 / 29)
    L = 116 * f[..., 1] - 16
    return np.stack([L, 0.01 * L * (500 * (f[..., 0] - f[..., 1])), 0.01 * L * (200 * (f[..., 1] - f[..., 2]))], axis=-1)


def hyab(a, b):
    d = a - b
    return np.abs(d[..., 0]) + np.sqrt(d[..., 1] ** 2 + d[..., 2] ** 2)


def cmax():
    """flip_loss.py:82-84"""
    return float(hyab(linrgb_to_hunt_lab(np.array([0.0, 1.0, 0.0])), linrgb_to_hunt_lab(np.array([0.0, 0.0, 1.0]))) ** QC)


def correlate_replicate(plane, table):
    """F.conv2d(F.pad(plane, r, mode='replicate'), table): cross-correlation of [h, w] with [2r+1, 2r+1], float64"""
    t = np.asarray(table, np.float64)
    r = t.shape[0] // 2
    h, w = plane.shape
    p = np.pad(plane, r, mode="edge")
    out = np.zeros((h, w), np.float64)
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            out += t[i, j] * p[i:i + h, j:j + w]
    return out


def flip_map(test, ref, ppd=None):
    """Error map [h, w] float64 of two [h, w, 3] sRGB images (compute_flip, flip_loss.py:61-105)."""
    ppd = DEFAULT_PPD if ppd is None or ppd <= 0 else float(ppd)
    test, ref = np.asarray(test, np.float64), np.asarray(ref, np.float64)
    assert test.shape == ref.shape and test.ndim == 3 and test.shape[2] == 3, (test.shape, ref.shape)
    opp = [srgb_to_ycxcz(test), srgb_to_ycxcz(ref)]

    # colour pipeline
    tabs = [spatial_filter_table(ppd, ch) for ch in ("A", "RG", "BY")]
    lab = []
    for o in opp:
        f = np.stack([correlate_replicate(o[..., c], tabs[c]) for c in range(3)], axis=-1)
        fy = (f[..., 0] + 16) / 116                                               # 'ycxcz2xyz'
        xyz = np.stack([fy + f[..., 1] / 500, fy, fy - f[..., 2] / 200], axis=-1) * ILLUM
        lab.append(linrgb_to_hunt_lab(np.clip(xyz @ A_INV.T, 0.0, 1.0)))
    e = hyab(lab[0], lab[1]) ** QC
    cm = cmax()
    pcc = PC * cm
    with np.errstate(invalid="ignore"):
        dc = np.where(e < pcc, (PT / pcc) * e, PT + ((e - pcc) / (cm - pcc)) * (1.0 - PT))

    # feature pipeline
    edge, point = feature_filter_table(ppd, "edge"), feature_filter_table(ppd, "point")
    norms = []
    for o in opp:
        y = (o[..., 0] + 16) / 116
        norms.append([np.sqrt(correlate_replicate(y, t) ** 2 + correlate_replicate(y, t.T) ** 2) for t in (edge, point)])
    d = np.maximum(np.abs(norms[0][0] - norms[1][0]), np.abs(norms[0][1] - norms[1][1]))
    df = np.clip(((1 / np.sqrt(2)) * d) ** QF, 0.0, 1.0)
    with np.errstate(invalid="ignore"):
        return np.power(dc, 1 - df)      # 0 ** 0 = 1, as torch.pow


def flip(test, ref, ppd=None):
    """(mean, map)"""
    m = flip_map(test, ref, ppd)
    return float(np.mean(m)), m


# ---- fixtures of tools/gen_flip_golden.py -----------------------------------------------------------------------------------------------

FIXTURES = ["flip_1x1", "flip_7x5", "flip_130x9", "flip_32x32", "flip_33x33", "flip_37x23", "flip_97x61", "flip_64x48_ppd30",
            "flip_45x41_ppd140"]
_cache = {}


def load_fixture(name):
    """{test, ref [h,w,3] fp32; ref_map [h,w] fp32, ref_mean: the reference's own; ppd; meta; ppd_arg: None for the default;
    map64, mean64: this module's restatement} -- computed once per process, shared, not to be written to."""
    if name not in _cache:
        import json
        import os
        z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")))
        z["meta"] = json.loads(bytes(z["meta"]).decode())
        z["ppd"] = float(z["ppd"])
        z["ppd_arg"] = None if z["meta"]["default_ppd"] else z["ppd"]
        z["mean64"], z["map64"] = flip(z["test"], z["ref"], z["ppd_arg"])
        for v in z.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = z
    return _cache[name]
