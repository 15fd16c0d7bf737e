"""Times an adaptively supersampled frame beside the full supersampled still and one plain render of the same build in the same process,
for profiles/adaptive_aa_measured.md: bench.py's default workload (config 2's model: N 8, threshold 0.2, bf16 shading, split-fp16
sampling) at 800 x 800 and 1920 x 1080, s = 2 and 3, contrast thresholds 0.05 / 0.1 / 0.2.

The three kinds of frame are timed on the device images alone (no download), alternated: every repetition runs the plain render, the full
S x S still and the adaptive frame of each threshold once, in that order, and the table gives the median and the spread (min .. max) of
--steps repetitions after --warmup.  Times are the host's wall clock around work that ends synchronised.  The contrast kernel alone is
timed with HIP events on the context's stream (no counter passed, so nothing but the launch lies between them).  Per setting also: the
flagged fraction f, the adaptive frame against (1 + s^2 f) plain frames -- profiles/masked_measured.md's rule: a masked pass costs the
full frame's per-ray cost times its rays, plus a fixed cost per pass that the rule leaves out -- and the fp32 PSNR of the adaptive and of
the plain frame against the full supersampled still.  Before anything is timed the device-side loop used here is checked against
NeuralRenderer.render_supersampled_adaptive / render_supersampled byte for byte.

    python tools/measure_adaptive_aa.py [--sizes 800x800 1920x1080] [--steps 10] [--warmup 2] [--out profiles/adaptive_aa_measured.md] [--json FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import adanerf_amd                      # noqa: E402
import bench                            # noqa: E402
from adanerf_amd import renderer as R   # noqa: E402
from measure_reproject import Hip       # noqa: E402

SCALES = (2, 3)
THRESHOLDS = (0.05, 0.1, 0.2)


def psnr(a, b):
    """fp32 images clamped to the display range, as the evaluator scores them against 8-bit ground truth"""
    a, b = np.clip(np.nan_to_num(a.astype(np.float64)), 0, 1), np.clip(np.nan_to_num(b.astype(np.float64)), 0, 1)
    mse = float(np.mean((a - b) ** 2))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def spread(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def measure(model_dir, w, h, steps, warmup, hip):
    stream, e0, e1 = hip.make("hipStreamCreate"), hip.make("hipEventCreate"), hip.make("hipEventCreate")
    n = w * h
    try:
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(model_dir, w, h)) as r:
            r.set_stream(stream.value)
            r.set_camera(np.array(list(r.info.view_cell_center), np.float32), np.eye(3, dtype=np.float32))
            out8, rgb, stage, total, d_mask = (r.empty((n, 4), np.uint8), r.empty((n, 3), np.float32), r.empty((n, 3), np.float32),
                                               r.empty((n, 3), np.float32), r.empty((n,), np.uint8))

            def plain():
                r.render(out8, rgb)
                r.sync()

            def full(s):
                for k, (dx, dy) in enumerate(R.subpixel_grid(s)):
                    r.set_pixel_offset(dx, dy)
                    r.render(None, stage)
                    r.accumulate_device(stage, n, total, first=k == 0)
                r.set_pixel_offset(0.0, 0.0)
                r.resolve_mean_device(total, n, s * s, out8, rgb)
                r.sync()

            def adaptive(s, thr):
                """the loop of NeuralRenderer.render_supersampled_adaptive on this tool's images, without the downloads; returns the flagged count"""
                r.render(out8, rgb)
                rc, flagged = r.contrast_mask(rgb, w, h, thr, d_mask)
                r._check(rc)
                if flagged:
                    for k, (dx, dy) in enumerate(R.subpixel_grid(s)):
                        r.set_pixel_offset(dx, dy)
                        r.render_masked(d_mask, 1, None, stage)
                        r.accumulate_masked_device(stage, d_mask, 1, n, total, first=k == 0)
                    r.set_pixel_offset(0.0, 0.0)
                    r.resolve_mean_masked_device(total, d_mask, 1, n, s * s, out8, rgb)
                r.sync()
                return flagged

            def wall(fn):
                t0 = time.perf_counter()
                fn()
                return (time.perf_counter() - t0) * 1e3

            # the frames themselves, and this tool's loops against the host's methods
            plain()
            plain_rgb = rgb.numpy()
            stills, frames, fractions = {}, {}, {}
            for s in SCALES:
                full(s)
                stills[s] = rgb.numpy()
                host_rgb, host_rgba, _ = r.render_supersampled(s)
                assert np.array_equal(host_rgb.view(np.uint32), stills[s].view(np.uint32)), "the tool's supersampling loop is not render_supersampled's"
                for thr in THRESHOLDS:
                    flagged = adaptive(s, thr)
                    frames[s, thr], fractions[s, thr] = rgb.numpy(), flagged / float(n)
                    host = r.render_supersampled_adaptive(s, thr)
                    assert host[3] == flagged and np.array_equal(host[0].view(np.uint32), frames[s, thr].view(np.uint32)) and \
                        np.array_equal(host[1], out8.numpy()), "the tool's adaptive loop is not render_supersampled_adaptive's"
                    m = host[2] == 0
                    assert np.array_equal(frames[s, thr].view(np.uint32)[m], stills[s].view(np.uint32)[m]) and \
                        np.array_equal(frames[s, thr].view(np.uint32)[~m], plain_rgb.view(np.uint32)[~m]), "the adaptive frame breaks its contract"

            # the contrast kernel alone: events around the launch, the image of the plain frame
            plain()
            kernel = {}
            for thr in THRESHOLDS:
                ev = [hip.timed(stream, e0, e1, lambda: r._check(r.contrast_mask(rgb, w, h, thr, d_mask, count=False)[0])) for _ in range(warmup + 20)][warmup:]
                kernel[thr] = spread(ev)

            # alternated: one repetition runs every kind of frame once
            t_plain, t_full, t_ada = [], {s: [] for s in SCALES}, {k: [] for k in frames}
            for rep in range(warmup + steps):
                a = wall(plain)
                b = {s: wall(lambda: full(s)) for s in SCALES}
                c = {(s, thr): wall(lambda: adaptive(s, thr)) for s in SCALES for thr in THRESHOLDS}
                if rep >= warmup:
                    t_plain.append(a)
                    for s in SCALES:
                        t_full[s].append(b[s])
                    for k in c:
                        t_ada[k].append(c[k])
            rows = []
            for s in SCALES:
                for thr in THRESHOLDS:
                    f = fractions[s, thr]
                    rows.append(dict(s=s, threshold=thr, fraction=f, kernel=kernel[thr], adaptive=spread(t_ada[s, thr]), full=spread(t_full[s]),
                                     rule_ms=(1.0 + s * s * f) * statistics.median(t_plain), psnr_adaptive=psnr(frames[s, thr], stills[s]),
                                     psnr_plain=psnr(plain_rgb, stills[s])))
            return dict(width=w, height=h, rays=n, plain=spread(t_plain), settings=rows)
    finally:
        hip.lib.hipEventDestroy(e0)
        hip.lib.hipEventDestroy(e1)
        hip.lib.hipStreamDestroy(stream)


def markdown(results, steps, warmup):
    t = lambda x: "%.3f (%.3f .. %.3f)" % (x["median_ms"], x["min_ms"], x["max_ms"])      # noqa: E731
    db = lambda v: "inf" if v == float("inf") else "%.2f dB" % v      # noqa: E731
    out = ["# Adaptive supersampling: measured cost", "",
           "One session on one MI355X, library sources `%s` (`adanerf_amd.build.source_hash()`), `tools/measure_adaptive_aa.py --steps %d --warmup %d`.  "
           "Workload: `bench.py`'s default (config 2's model: N 8, threshold 0.2, bf16 shading, split-fp16 sampling), RGBA8 and fp32 colour "
           "outputs, no aux maps, the camera at the view-cell centre.  Frame times: the host's wall clock around work that ends synchronised, "
           "device images only; every repetition runs the plain render, both full stills and all six adaptive frames once, in turn; median "
           "(min .. max) of %d repetitions after %d warm-ups.  Contrast kernel: HIP events around the launch alone, median (min .. max) of 20." %
           (adanerf_amd.build.source_hash(), steps, warmup, steps, warmup), ""]
    for res in results:
        w, h, n = res["width"], res["height"], res["rays"]
        out += ["## %d x %d (%d rays)" % (w, h, n), "", "One plain render (`adanerf_render`): %s ms." % t(res["plain"]), "",
                "| s | contrast threshold | flagged fraction f | contrast kernel ms | adaptive frame ms | full s x s still ms | adaptive / full | "
                "(1 + s^2 f) plain frames ms | adaptive / that | PSNR adaptive vs still | PSNR plain vs still |",
                "|---|---|---|---|---|---|---|---|---|---|---|"]
        for x in res["settings"]:
            out.append("| %d | %.2f | %.2f %% | %s | %s | %s | %.3f | %.3f | %.3f | %s | %s |" % (
                x["s"], x["threshold"], 100.0 * x["fraction"], "%.4f (%.4f .. %.4f)" % (x["kernel"]["median_ms"], x["kernel"]["min_ms"], x["kernel"]["max_ms"]),
                t(x["adaptive"]), t(x["full"]), x["adaptive"]["median_ms"] / x["full"]["median_ms"], x["rule_ms"],
                x["adaptive"]["median_ms"] / x["rule_ms"], db(x["psnr_adaptive"]), db(x["psnr_plain"])))
        cheaper = [x for x in res["settings"] if x["adaptive"]["median_ms"] < x["full"]["median_ms"]]
        out += ["", "The adaptive frame is cheaper than the full still in %d of %d settings%s." % (
            len(cheaper), len(res["settings"]),
            "" if len(cheaper) == len(res["settings"]) else ": not at " + ", ".join("s = %d / %.2f" % (x["s"], x["threshold"]) for x in res["settings"] if x not in cheaper)), ""]
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", nargs="+", default=["800x800", "1920x1080"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="the tables as markdown")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    adanerf_amd.build_library()
    hip = Hip()
    _, _, n, thr, tag = bench.WORKLOADS["config2"]
    results = []
    with tempfile.TemporaryDirectory() as td:
        bench.build_model_dir(td, tag, n, thr)
        for size in a.sizes:
            w, h = (int(v) for v in size.split("x"))
            results.append(measure(td, w, h, a.steps, a.warmup, hip))
    text = markdown(results, a.steps, a.warmup)
    print(text, flush=True)
    for path, body in ((a.out, text), (a.json, json.dumps(dict(steps=a.steps, warmup=a.warmup, source_hash=adanerf_amd.build.source_hash(), results=results), indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(body + "\n")


if __name__ == "__main__":
    main()
