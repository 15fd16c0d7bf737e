#!/usr/bin/env python3
"""Times a wide network: a random-init model directory with an 8 x 256 sampling net and an 8 x 512 / skip 4 shading net (the staged
16-bit kernel at width 512 in bf16, the wide fp32 form in fp32), frames of 800 x 800 at N = 8.  Prints one JSON line per precision:
FPS, the mean per-frame stage timings, and the shading stage's `frac` = algorithmic FLOP / (ms_shade_mlp x 2.5 PFLOP/s, the nominal
bf16 / fp16 MFMA peak; fp32 MFMA peaks at 1/16 of it).

Usage:  python tools/bench_wide.py [--frames 200] [--warmup 10] [--precisions bf16,fp32] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import adanerf_oracle as O  # noqa: E402

import adanerf_amd  # noqa: E402

PEAK_FLOPS = 2.5e15


def shading_flop_per_sample(wts):
    """2 x multiply-adds of the network's own (unpadded) layers"""
    macs = sum(int(np.prod(v.shape)) for k, v in wts.net1.items() if k.endswith(".weight"))
    return 2 * macs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--precisions", default="bf16,fp32")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    wts = O.synthetic_weights(11, oracle_bias=0.1, oracle_scale=0.3, layers=(8, 8), widths=(256, 512), skip1=4)
    flop = shading_flop_per_sample(wts)
    pose = np.array(sc.view_cell_center, dtype=np.float32)
    rot = O.camera_rotation(100.0, 0.0)
    lines = []
    with tempfile.TemporaryDirectory() as td:
        O.write_model_dir(td, sc, wts)
        for prec in args.precisions.split(","):
            with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(td, args.size, args.size), precision=prec) as r:
                r.set_camera(pose, rot)
                rgb = r.empty((args.size * args.size, 3), np.float32)
                for _ in range(args.warmup):
                    r.render(None, rgb, stats=True)
                acc = dict(ms_total=0.0, ms_sample_mlp=0.0, ms_compact=0.0, ms_shade_mlp=0.0)
                samples = 0
                t0 = time.perf_counter()
                for _ in range(args.frames):
                    st = r.render(None, rgb, stats=True)
                    for k in acc:
                        acc[k] += float(getattr(st, k))
                    samples += int(st.total_samples)
                wall = time.perf_counter() - t0
                assert np.isfinite(rgb.numpy()).all()
            ms = {k: v / args.frames for k, v in acc.items()}
            spf = samples / args.frames
            res = dict(tool="bench_wide", precision=prec, size=args.size, frames=args.frames, nets="8x256 sampling / 8x512 skip4 shading",
                       fps=args.frames / wall, samples_per_frame=spf, shade_flop_per_sample=flop,
                       shade_tflops=flop * spf / (ms["ms_shade_mlp"] * 1e-3) / 1e12,
                       frac=flop * spf / (ms["ms_shade_mlp"] * 1e-3 * PEAK_FLOPS), **ms)
            print(json.dumps(res), flush=True)
            lines.append(res)
    if len(lines) == 2 and {l["precision"] for l in lines} == {"bf16", "fp32"}:
        b = next(l for l in lines if l["precision"] == "bf16")
        f = next(l for l in lines if l["precision"] == "fp32")
        print(json.dumps(dict(tool="bench_wide", shade_speedup_bf16_over_fp32=f["ms_shade_mlp"] / b["ms_shade_mlp"])), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            for l in lines:
                fh.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
