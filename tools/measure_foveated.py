"""Times a frame at a foveated ray density beside adanerf_render of the same build in the same process, for
profiles/foveated_density_measured.md: bench.py's default workload (config 2's model: N 8, threshold 0.2, bf16 shading, split-fp16
sampling) at 800 x 800 and 1920 x 1080, the gaze at the frame centre, the settings 120:1,300:2,4 and 200:1,500:2,4 and one with a stride-8
outside (120:1,250:2,400:4,8).

Per setting, median of --steps calls after --warmup, each both as the wall time on the host around work that ends synchronised and as HIP
events on the context's stream: the mask kernel (adanerf_foveate_density), the fill kernel (adanerf_fill_density over RGBA8 + fp32, no
counter), the masked render of the lattice alone, and the whole foveated frame (masked render + fill; the mask is filled once per gaze, so
it is listed but not part of the frame).  adanerf_render of the same context writes the same two outputs.  Also: the rendered fraction, the
frame predicted from profiles/masked_measured.md's rule (this session's fixed cost of a masked call + this session's per-ray cost of the
full frame x rendered rays + the fill), and the 8-bit PSNR of the reconstructed frame against the full frame over the whole image and
inside the innermost ring, where every pixel is rendered and it must be infinite.

    python tools/measure_foveated.py [--sizes 800x800 1920x1080] [--steps 20] [--warmup 5] [--out profiles/foveated_density_measured.md] [--json FILE.json]
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

SETTINGS = ["120:1,300:2,4", "200:1,500:2,4", "120:1,250:2,400:4,8"]


def psnr8(a, b):
    mse = float(np.mean((a[:, :3].astype(np.float64) / 255.0 - b[:, :3].astype(np.float64) / 255.0) ** 2))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def measure(model_dir, w, h, steps, warmup, hip):
    stream, e0, e1 = hip.make("hipStreamCreate"), hip.make("hipEventCreate"), hip.make("hipEventCreate")
    n = w * h
    med = statistics.median
    try:
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(model_dir, w, h)) as r:
            r.set_stream(stream.value)
            r.set_camera(np.array(list(r.info.view_cell_center), np.float32), np.eye(3, dtype=np.float32))
            out8, rgb, d_mask = r.empty((n, 4), np.uint8), r.empty((n, 3), np.float32), r.empty((n,), np.uint8)
            gaze = (0.5 * w, 0.5 * h)

            def timed(fn):
                """fn enqueues (or runs) the work; the wall clock stops after a synchronisation"""
                wall, ev = [], []
                for _ in range(warmup + steps):
                    t0 = time.perf_counter()
                    ev.append(hip.timed(stream, e0, e1, fn))      # ends in hipEventSynchronize of the event behind the work
                    wall.append((time.perf_counter() - t0) * 1e3)
                wall, ev = wall[warmup:], ev[warmup:]
                return dict(wall_ms=med(wall), wall_min_ms=min(wall), wall_max_ms=max(wall), event_ms=med(ev))

            full = timed(lambda: r.render(out8, rgb, stats=True))
            full_frame = out8.numpy()
            d_mask.upload(np.ones(n, np.uint8))
            empty = timed(lambda: r.render_masked(d_mask, 1, rgba8=out8, rgb=rgb))
            rows = []
            for spec in SETTINGS:
                rings = R.parse_fovea_density(spec)
                mask_t = timed(lambda: r._check(r.foveate_density_device(gaze, rings, d_mask)))
                mask = d_mask.numpy()
                assert np.array_equal(mask, R.density_mask(w, h, gaze, rings)), "device mask differs from the host mask"
                rendered = int(np.count_nonzero(mask == 0))
                lattice_t = timed(lambda: r.render_masked(d_mask, 1, rgba8=out8, rgb=rgb))
                fill_t = timed(lambda: r._check(r.fill_density_device(d_mask, w, h, rgb, None, None, out8, count=False)[0]))

                def frame():
                    m, _ = r.render_masked(d_mask, 1, rgba8=out8, rgb=rgb)
                    r._check(r.fill_density_device(d_mask, w, h, rgb, None, None, out8, count=False)[0])
                    return m
                frame_t = timed(frame)
                out8.upload(np.zeros((n, 4), np.uint8))      # the scored frame starts from nothing: every pixel is rendered or filled
                rgb.upload(np.zeros((n, 3), np.float32))
                assert frame() == rendered
                rc, unfilled = r.fill_density_device(d_mask, w, h, rgb, None, None, out8)
                r._check(rc)
                got = out8.numpy()
                yy, xx = np.divmod(np.arange(n), w)
                q = (2 * xx + 1 - int(round(2 * gaze[0]))) ** 2 + (2 * yy + 1 - int(round(2 * gaze[1]))) ** 2
                inner = q <= 4 * rings[0][0] ** 2 if len(rings) > 1 and rings[0][1] == 1 else np.zeros(n, bool)
                predicted = empty["wall_ms"] + full["wall_ms"] / n * rendered + fill_t["event_ms"]
                rows.append(dict(spec=spec, rendered=rendered, fraction=rendered / n, unfilled=unfilled, mask=mask_t, lattice=lattice_t, fill=fill_t,
                                 frame=frame_t, predicted_ms=predicted, psnr_whole=psnr8(got, full_frame),
                                 psnr_inner=psnr8(got[inner], full_frame[inner]) if inner.any() else None, inner_pixels=int(inner.sum())))
            return dict(width=w, height=h, rays=n, render=full, masked_empty=empty, settings=rows)
    finally:
        hip.lib.hipEventDestroy(e0)
        hip.lib.hipEventDestroy(e1)
        hip.lib.hipStreamDestroy(stream)


def markdown(results, steps, warmup):
    out = ["# Foveated ray density: measured cost", "",
           "One session on one MI355X, library sources `%s` (`adanerf_amd.build.source_hash()`), `tools/measure_foveated.py --steps %d --warmup %d`: "
           "medians of %d calls after %d warm-ups.  Workload: `bench.py`'s default (config 2's model: N 8, threshold 0.2, bf16 shading, split-fp16 "
           "sampling), RGBA8 and fp32 colour outputs, no aux maps, gaze at the frame centre.  wall: host clock around the work, which ends "
           "synchronised; events: HIP events on the context's stream around it." % (adanerf_amd.build.source_hash(), steps, warmup, steps, warmup), ""]
    t = lambda x: "%.4f (%.4f .. %.4f) / %.4f" % (x["wall_ms"], x["wall_min_ms"], x["wall_max_ms"], x["event_ms"])      # noqa: E731
    for res in results:
        w, h, n = res["width"], res["height"], res["rays"]
        f, e = res["render"], res["masked_empty"]
        out += ["## %d x %d (%d rays)" % (w, h, n), "",
                "`adanerf_render`: %s ms (wall median (min .. max) / events).  A masked call that selects nothing: %s ms." % (t(f), t(e)), "",
                "| setting | rendered | fraction | mask kernel | fill kernel | lattice alone (masked render) | foveated frame (masked render + fill) | frame / `adanerf_render` | predicted frame | PSNR whole | PSNR inner ring |",
                "|---|---|---|---|---|---|---|---|---|---|---|"]
        for x in res["settings"]:
            out.append("| `%s` | %d | %.1f %% | %s | %s | %s | %s | %.3f | %.3f | %.2f dB | %s |" % (
                x["spec"], x["rendered"], 100.0 * x["fraction"], t(x["mask"]), t(x["fill"]), t(x["lattice"]), t(x["frame"]),
                x["frame"]["wall_ms"] / f["wall_ms"], x["predicted_ms"], x["psnr_whole"],
                "-" if x["psnr_inner"] is None else ("inf (%d px)" % x["inner_pixels"] if x["psnr_inner"] == float("inf") else "%.2f dB" % x["psnr_inner"])))
        out += ["", "Every cell: wall ms median (min .. max) / events ms.  predicted frame = the empty masked call's wall + `adanerf_render`'s wall per ray x "
                "rendered rays + the fill's events, all of this session.  unfilled pixels: %s." % ", ".join(str(x["unfilled"]) for x in res["settings"]), ""]
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", nargs="+", default=["800x800", "1920x1080"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
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
