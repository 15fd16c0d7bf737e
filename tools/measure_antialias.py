"""Times the anti-aliasing stages beside a rendered frame of the same session, for profiles/antialias_measured.md: the area filter of
adanerf_present (ADANERF_PRESENT_AREA), adanerf_accumulate and adanerf_resolve_mean.  HIP events on the context's stream, median of --steps
single calls after --warmup, and the per-call time of a window of --burst back-to-back calls (the stages are short: a single call's time
includes the launch).  Also the report-only cross-check of the two supersampling paths on bench.py's default workload (config2's model):
the mean of the 2 x 2 grid at 400 x 400 against an 800 x 800 frame reduced by the area filter -- mathematically the same rays with
different rounding.

    python tools/measure_antialias.py [--steps 30] [--warmup 5] [--burst 50] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import adanerf_amd                      # noqa: E402
import bench                            # noqa: E402
from adanerf_amd import renderer as R   # noqa: E402
from measure_reproject import Hip       # noqa: E402


def timed(hip, stream, ev, call, steps, warmup, burst):
    single = [hip.timed(stream, ev[0], ev[1], call) for _ in range(warmup + steps)][warmup:]

    def many():
        for _ in range(burst):
            call()
    window = [hip.timed(stream, ev[0], ev[1], many) / burst for _ in range(3 + 5)][3:]
    return dict(median_ms=statistics.median(single), min_ms=min(single), max_ms=max(single), per_call_in_burst_ms=statistics.median(window))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    adanerf_amd.build_library()
    hip = Hip()
    _, _, n_samples, thr, tag = bench.WORKLOADS["config2"]
    res = dict(steps=a.steps, warmup=a.warmup, burst=a.burst, source_hash=adanerf_amd.build.source_hash())
    stream, ev = hip.make("hipStreamCreate"), (hip.make("hipEventCreate"), hip.make("hipEventCreate"))
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as td:
        bench.build_model_dir(td, tag, n_samples, thr)
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(td, 800, 800)) as r:
            r.set_stream(stream.value)
            pos, rot = np.array(list(r.info.view_cell_center), np.float32), np.eye(3, dtype=np.float32)
            r.set_camera(pos, rot)
            frames = [r.render_numpy()[2] for _ in range(a.warmup + a.steps)][a.warmup:]
            med = lambda f: statistics.median(getattr(s, f) for s in frames)
            res["render_800x800"] = dict(ms_total=med("ms_total"), ms_sample_mlp=med("ms_sample_mlp"), ms_compact=med("ms_compact"), ms_shade_mlp=med("ms_shade_mlp"),
                                         ms_composite=med("ms_composite"))
            tf, mhz = r.probe_mfma("relu")
            res["mfma_probe"] = dict(tflops=tf, clock_mhz=mhz)
            # accumulate / resolve at 800 x 800, on the rendered frame
            n = 800 * 800
            total, px = r.empty((n, 3), np.float32), r.empty((n, 4), np.uint8)
            r.accumulate_device(r._o_rgb, n, total, True)
            res["accumulate_800x800"] = timed(hip, stream, ev, lambda: r.accumulate_device(r._o_rgb, n, total, False), a.steps, a.warmup, a.burst)
            res["accumulate_800x800"]["bytes"] = n * 3 * 4 * 3      # two reads, one write
            res["resolve_800x800"] = timed(hip, stream, ev, lambda: r.resolve_mean_device(total, n, 4, px, r._o_rgb), a.steps, a.warmup, a.burst)
            res["resolve_800x800"]["bytes"] = n * (12 + 12 + 4)
            for sw, sh, dw, dh in ((1600, 1600, 800, 800), (1920, 1080, 960, 540)):
                src = r.empty((sh * sw, 4), np.uint8).upload(rng.integers(0, 256, (sh * sw, 4), dtype=np.uint8))
                dst = r.empty((dh * dw, 4), np.uint8)
                key = "present_area_%dx%d_to_%dx%d" % (sw, sh, dw, dh)
                res[key] = timed(hip, stream, ev, lambda: r.present_device(src, sw, sh, dst, dw, dh, filter="area"), a.steps, a.warmup, a.burst)
                res[key]["bytes"] = 4 * (sw * sh + dw * dh)
                res[key + "_nearest"] = timed(hip, stream, ev, lambda: r.present_device(src, sw, sh, dst, dw, dh, filter="nearest"), a.steps, a.warmup, a.burst)
            for key in [k for k in res if k.startswith(("accumulate", "resolve", "present"))]:
                res[key]["fraction_of_frame"] = res[key]["median_ms"] / res["render_800x800"]["ms_total"]
                print("%s: %.4f ms (min %.4f, max %.4f; %.4f ms per call in a burst of %d) = %.3f %% of the rendered 800x800 frame (%.3f ms)" % (
                    key, res[key]["median_ms"], res[key]["min_ms"], res[key]["max_ms"], res[key]["per_call_in_burst_ms"], a.burst,
                    100.0 * res[key]["fraction_of_frame"], res["render_800x800"]["ms_total"]), flush=True)
            # the two supersampling paths: 800 x 800 reduced by the area filter ...
            _, big, _ = r.render_numpy()
            small = r.present(400, 400, filter="area").reshape(-1, 4)
            # ... against the mean of the 2 x 2 grid at 400 x 400
            r.set_frame_size(400, 400)
            _, grid, st = r.render_supersampled(2)
            _, centre, _ = r.render_numpy()
            psnr = lambda x, y: float(-10.0 * np.log10(max(np.mean((x[:, :3].astype(np.float64) / 255.0 - y[:, :3].astype(np.float64) / 255.0) ** 2), 1e-30)))
            diff = grid[:, :3].astype(np.int32) - small[:, :3].astype(np.int32)
            res["cross_check_400x400"] = dict(psnr_grid_vs_area=psnr(grid, small), differing_bytes=float(np.mean(diff != 0)), max_abs_difference=int(np.abs(diff).max()),
                                              differing_by_more_than_1=float(np.mean(np.abs(diff) > 1)), psnr_centre_vs_area=psnr(centre, small),
                                              psnr_centre_vs_grid=psnr(centre, grid), ms_total_4_renders=st.ms_total)
            print("cross-check 400x400: %s" % json.dumps(res["cross_check_400x400"]), flush=True)
    print("rendered 800x800 frame: %s; MFMA probe %.1f TFLOP/s at %.0f MHz" % (json.dumps(res["render_800x800"]), tf, mhz), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
