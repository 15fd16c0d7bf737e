"""Writes tests/golden/flip_*.npz: FLIP fixtures pinned to the reference's own implementation.

The reference's src/util/flip_loss.py is imported BY PATH (nothing of it is copied here) and run on the CPU: it hard-codes .cuda()
and device='cuda', so torch.Tensor.cuda is patched to return the tensor itself and the module sees a `torch` proxy whose zeros()
drops the device argument.  Each fixture holds the two input images, the reference's fp32 error map and mean, pixels per degree
and a meta record with ``ref_fp32_residual`` / ``ref_fp32_residual_mean``: how far the reference's fp32 map / mean sit from the
float64 restatement tests/flip_reference.py on the same inputs -- the rounding error of the reference's own arithmetic, which the
tests scale their bounds from.

    python tools/gen_flip_golden.py [--reference /root/reference] [--out tests/golden] [--only flip_37x23,...]

Images are deterministic (np.random.RandomState): a smooth gradient, step edges, isolated bright points, a flat region where both
images agree exactly, and noise; the test image carries values below 0 and above 1 (the renderer's fp32 colour is unclamped).
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, width, height, pixels per degree or None for the reference's default)
FIXTURES = [("flip_1x1", 1, 1, None),                # degenerate image
            ("flip_7x5", 7, 5, None),                # smaller than either radius: the replicate pad covers everything
            ("flip_130x9", 130, 9, None),            # one dimension below the radius
            ("flip_32x32", 32, 32, None),            # the kernel's tile ...
            ("flip_33x33", 33, 33, None),            # ... and one more
            ("flip_37x23", 37, 23, None),            # ragged in both dimensions
            ("flip_97x61", 97, 61, None),            # several tiles, ragged edges
            ("flip_64x48_ppd30", 64, 48, 30.0),      # radii 5 and 4: run-time radii
            ("flip_45x41_ppd140", 45, 41, 140.0)]    # radii 19 and 18, the largest supported: the tile's LDS image exceeds 64 KB


def make_pair(w, h, seed):
    """(test, ref) float32 [h, w, 3]"""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    u, v = xx / max(w - 1, 1), yy / max(h - 1, 1)
    ref = np.stack([0.15 + 0.7 * u, 0.2 + 0.6 * v, 0.5 + 0.4 * np.sin(6.0 * u + 2.0 * v)], axis=-1)      # smooth gradients
    ref[:, w // 3:w // 3 + max(w // 6, 1), :] *= 0.35                                                     # vertical step edges
    ref[h // 2:h // 2 + max(h // 5, 1), :, 1] = 0.9                                                       # horizontal step edges, one channel
    flat = (slice(0, h // 4), slice(w - w // 4, w)) if min(w, h) >= 8 else (slice(0, 0), slice(0, 0))      # none in the smallest images
    ref[flat] = (0.25, 0.5, 0.75)                                                                         # flat region
    n_pts = max(1, (w * h) // 150)
    py, px = rs.randint(0, h, n_pts), rs.randint(0, w, n_pts)
    ref[py, px] = 1.0                                                                                     # isolated bright points
    ref = np.clip(ref + 0.02 * rs.standard_normal(ref.shape), 0.0, 1.0)                                   # noise
    ref[flat] = (0.25, 0.5, 0.75)

    test = ref.copy()
    test += 0.05 * rs.standard_normal(ref.shape) * (u[..., None] > 0.5)                                   # noisy right half
    test[:, : w // 2, :] = np.roll(ref, 1, axis=1)[:, : w // 2, :] * 1.05                                 # left half: edges shifted by a pixel
    test[py[::2], px[::2]] = ref[np.minimum(py[::2] + 1, h - 1), px[::2]]                                 # every other point missing
    test[rs.randint(0, h, n_pts), rs.randint(0, w, n_pts), rs.randint(0, 3, n_pts)] = -0.3                # below 0
    test[rs.randint(0, h, n_pts), rs.randint(0, w, n_pts), rs.randint(0, 3, n_pts)] = 1.6                 # above 1
    test[flat] = ref[flat]                                                                                # agrees exactly here
    return test.astype(np.float32), ref.astype(np.float32)


def load_reference_flip(reference_root):
    """The reference's FLIP class, runnable without a GPU."""
    import torch
    torch.set_num_threads(1)      # one summation order
    path = os.path.join(reference_root, "src", "util", "flip_loss.py")
    spec = importlib.util.spec_from_file_location("reference_flip_loss", path)
    mod = importlib.util.module_from_spec(spec)
    torch.Tensor.cuda = lambda self, *a, **k: self

    class TorchOnCpu:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def zeros(*a, **k):
            k.pop("device", None)
            return torch.zeros(*a, **k)

    spec.loader.exec_module(mod)
    mod.torch = TorchOnCpu()
    return mod


def reference_map(mod, test, ref, ppd):
    """fp32 [h, w] error map and mean, argument order of src/evaluate.py:144"""
    import torch
    flip = mod.FLIP()
    t = torch.from_numpy(test).permute(2, 0, 1)[None].contiguous()
    r = torch.from_numpy(ref).permute(2, 0, 1)[None].contiguous()
    with torch.no_grad():
        m = flip.compute_flip(t, r, flip.pixels_per_degree if ppd is None else ppd)
        mean = torch.mean(m)
    assert m.dtype == torch.float32 and tuple(m.shape) == (1, 1) + test.shape[:2], (m.dtype, m.shape)
    return m[0, 0].numpy().copy(), np.float32(mean.item())


def generate(name, w, h, ppd, mod):
    import flip_reference as F
    test, ref = make_pair(w, h, seed=1000 + 7 * w + h)
    rmap, rmean = reference_map(mod, test, ref, ppd)
    mean64, map64 = F.flip(test, ref, ppd)
    meta = dict(name=name, width=w, height=h, default_ppd=ppd is None, radii=list(F.radii(F.DEFAULT_PPD if ppd is None else ppd)),
                ref_fp32_residual=float(np.max(np.abs(rmap.astype(np.float64) - map64))),
                ref_fp32_residual_mean=float(abs(float(rmean) - mean64)),
                source="src/util/flip_loss.py FLIP.compute_flip on the CPU, arguments as src/evaluate.py:144")
    return dict(test=test, ref=ref, ref_map=rmap, ref_mean=np.float32(rmean), ppd=np.float64(F.DEFAULT_PPD if ppd is None else ppd),
                meta=np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="")
    a = ap.parse_args(argv)
    mod = load_reference_flip(a.reference)
    only = set(filter(None, a.only.split(",")))
    os.makedirs(a.out, exist_ok=True)
    for name, w, h, ppd in FIXTURES:
        if only and name not in only:
            continue
        z = generate(name, w, h, ppd, mod)
        np.savez(os.path.join(a.out, name + ".npz"), **z)
        meta = json.loads(bytes(z["meta"]).decode())
        print("%-20s mean %.6f  radii %s  ref_fp32_residual %.3e  mean %.3e" % (name, float(z["ref_mean"]), meta["radii"], meta["ref_fp32_residual"],
                                                                                 meta["ref_fp32_residual_mean"]))


if __name__ == "__main__":
    main()
