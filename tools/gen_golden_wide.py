#!/usr/bin/env python3
"""Writes the wide-network fixtures tests/golden/syn_w320_w512_skip4.npz and syn_w256_w384_skips_1_4.npz: hidden widths
257..512 (run zero-padded to 512, pack.cpp pad_width) through the reference's own model classes (BaseNet / NeRF,
src/models.py:18-82, 199-277), shaped like oracle/gen_golden.py's other synthetic cases (400 x 400 scene, a 24 x 16 crop,
weights regenerated from the seed by tests/conftest.py case_weights).

Needs the reference checkout gen_golden.py imports (build container only).

Usage:  python tools/gen_golden_wide.py [--out DIR]
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import adanerf_oracle as O  # noqa: E402
import gen_golden as G  # noqa: E402

CASES = [
    # sampling 4 x 320 (padded to 512), shading 8 x 512 with the shipped skip after layer 4
    ("syn_w320_w512_skip4", dict(seed=41, layers=[4, 8], widths=[320, 512], skip1=4, oracle_bias=0.1, oracle_scale=0.3)),
    # sampling 8 x 256 (the existing kernels), shading 6 x 384 (padded to 512) with two skips
    ("syn_w256_w384_skips_1_4", dict(seed=42, layers=[8, 6], widths=[256, 384], skip1=[1, 4], oracle_bias=0.1, oracle_scale=0.3)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write into this directory instead of tests/golden")
    args = ap.parse_args()
    if args.out:
        G.GOLD = os.path.abspath(args.out)
    os.makedirs(G.GOLD, exist_ok=True)
    R = G.import_reference()
    R.torch.manual_seed(0)
    base = G.classroom_scene(8, 0.65)
    pose = np.array(base.view_cell_center, dtype=np.float32)
    rot = O.camera_rotation(100.0, 0.0)
    for name, syn in CASES:
        sc = dataclasses.replace(base, ray_sample_input=0)
        wts = O.synthetic_weights(syn["seed"], n_in0=sc.n_in0, oracle_bias=syn["oracle_bias"], oracle_scale=syn["oracle_scale"],
                                  layers=tuple(syn["layers"]), widths=tuple(syn["widths"]), skip1=syn["skip1"])
        dirs = G.subset_dirs(400, 400, sc.fov, 12, 20, 24, 16, 16)
        tc = G.build_reference(R, sc, wts, 400, 400)
        ref = G.run_reference(R, tc, dirs, pose, rot)
        G.save_case(name, sc, dict(w=400, h=400, crop=[12, 20, 24, 16, 16], yaw=100.0, pitch=0.0, syn=dict(syn, n_in0=sc.n_in0)),
                    dirs, pose, rot, ref, 8, "synthetic")


if __name__ == "__main__":
    main()
