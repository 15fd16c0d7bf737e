"""Times adanerf_render_masked beside adanerf_render of the same build in the same process, for profiles/masked_measured.md: bench.py's
default workload (config 2's model: N 8, threshold 0.2, bf16 shading, split-fp16 sampling) at 800 x 800 and 1920 x 1080, M / R = 0.1 %, 1 %,
5 %, 25 %, 50 %, 100 % of the frame, each with a uniformly random mask and a clustered one -- the hole mask of a reprojection step (fill
off) on the path profiles/reproject_measured.md used (camera at the view-cell centre, destination a tenth of the view cell away), cut off
after M holes in pixel order and, where the warp has fewer holes than M, filled up with whole rows from the top.

Per case, median of --steps calls after --warmup: the wall time of the call on the host (it ends in a synchronisation), HIP events on the
context's stream around the call, and the per-stage times of its adanerf_stats.  The list kernels on their own are the event time of a call
that selects nothing (M = 0: mask to bit words, bit words to list, the 4-byte read-back); the scatter is what remains of a call's event time
after its stats' first-launch-to-last-kernel span and that list time.  Derived: the fixed cost (M -> 0), the slope per ray against the
full frame's per-ray cost, the 100 % case's overhead over adanerf_render.  Also: hole fractions of the warp, and the 8-bit PSNR of the
warped, warped + holes and warped + unsourced frames against the frame rendered at the destination pose.

    python tools/measure_masked.py [--sizes 800x800 1920x1080] [--steps 20] [--warmup 5] [--out profiles/masked_measured.md] [--json FILE.json]
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
from measure_reproject import Hip       # noqa: E402

FRACTIONS = [0.001, 0.01, 0.05, 0.25, 0.5, 1.0]
STAGES = ("ms_total", "ms_sample_mlp", "ms_compact", "ms_shade_mlp", "ms_composite")


def random_mask(n, m, seed=1):
    mask = np.ones(n, np.uint8)
    mask[np.random.default_rng(seed).permutation(n)[:m]] = 0
    return mask


def clustered_mask(holes, w, m):
    """the warp's holes (bool [n]) in pixel order, the first m of them; fewer than m holes: whole rows from the top until m pixels are selected"""
    n = holes.size
    idx = np.flatnonzero(holes)[:m]
    mask = np.ones(n, np.uint8)
    mask[idx] = 0
    missing = m - idx.size
    if missing > 0:
        rest = np.flatnonzero(mask == 1)[:missing]      # pixel order: rows from the top, their holes already taken
        mask[rest] = 0
    return mask


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
            r.enable_reprojection()
            pos = np.array(list(r.info.view_cell_center), np.float32)
            rot = np.eye(3, dtype=np.float32)
            dst = (pos + np.float32(0.1) * np.array(list(r.info.view_cell_size), np.float32)).astype(np.float32)
            # ---- the warp of the source frame: its holes, and what re-rendering them is worth
            r.set_camera(dst, rot)
            fresh = r.render_numpy()[1]
            r.set_camera(pos, rot)
            r.render_numpy()
            warped, wmask, holes_fill = r.reproject(dst, rot)
            _, bare_mask, holes_bare = r.reproject(dst, rot, fill=False)
            with_holes, _, _, m_holes = r.reproject_rerender(dst, rot, "holes")
            unsourced, _, _, m_unsourced = r.reproject_rerender(dst, rot, "unsourced")
            quality = dict(holes_filled=holes_fill, holes_unfilled=holes_bare, rerendered_holes=m_holes, rerendered_unsourced=m_unsourced,
                           psnr_warped=psnr8(warped, fresh), psnr_warped_holes=psnr8(with_holes, fresh), psnr_warped_unsourced=psnr8(unsourced, fresh))
            # ---- adanerf_render and the masked call, same context, same outputs (RGBA8 only, no aux maps), camera at the destination
            r.set_aux_outputs(None, None)
            out = r.empty((n, 4), np.uint8)
            d_mask = r.empty((n,), np.uint8)

            def timed(fn):
                wall, ev, stats = [], [], []
                for _ in range(warmup + steps):
                    t0 = time.perf_counter()
                    box = []
                    ev.append(hip.timed(stream, e0, e1, lambda: box.append(fn())))
                    wall.append((time.perf_counter() - t0) * 1e3)
                    stats.append(box[0])
                wall, ev, stats = wall[warmup:], ev[warmup:], stats[warmup:]
                row = dict(wall_ms=med(wall), wall_min_ms=min(wall), wall_max_ms=max(wall), event_ms=med(ev))
                row.update({k: med(getattr(s, k) for s in stats) for k in STAGES})
                row["total_samples"] = int(stats[-1].total_samples)
                return row

            full = timed(lambda: r.render(out, None, stats=True))
            d_mask.upload(np.ones(n, np.uint8))
            empty = timed(lambda: r.render_masked(d_mask, 1, rgba8=out)[1])
            rows = []
            for f in FRACTIONS:
                m = max(1, int(round(f * n)))
                for kind, mask in (("random", random_mask(n, m)), ("clustered", clustered_mask(bare_mask == 0, w, m))):
                    assert int(np.count_nonzero(mask == 0)) == m
                    d_mask.upload(mask)
                    got_m = r.render_masked(d_mask, 1, rgba8=out)[0]
                    assert got_m == m, (got_m, m)
                    row = timed(lambda: r.render_masked(d_mask, 1, rgba8=out)[1])
                    row.update(fraction=f, kind=kind, rays=m, scatter_ms=row["event_ms"] - row["ms_total"] - empty["event_ms"])
                    rows.append(row)
            d_mask.upload(np.zeros(n, np.uint8))      # sanity: the 100 % call leaves adanerf_render's bytes
            r.render(out, None)
            want = out.numpy()
            r.render_masked(d_mask, 1, rgba8=out)
            same = bool(np.array_equal(want, out.numpy()))
            whole = {k: [x for x in rows if x["fraction"] == 1.0 and x["kind"] == k][0] for k in ("random", "clustered")}
            derived = dict(fixed_cost_wall_ms=empty["wall_ms"], list_kernels_event_ms=empty["event_ms"],
                           full_per_ray_us=1e3 * full["wall_ms"] / n,
                           slope_per_ray_us={k: 1e3 * (whole[k]["wall_ms"] - empty["wall_ms"]) / n for k in whole},
                           overhead_100pct_wall_ms={k: whole[k]["wall_ms"] - full["wall_ms"] for k in whole},
                           overhead_100pct={k: whole[k]["wall_ms"] / full["wall_ms"] - 1.0 for k in whole}, same_bytes_at_100pct=same)
            return dict(width=w, height=h, rays=n, render=full, masked_empty=empty, masked=rows, derived=derived, quality=quality)
    finally:
        hip.lib.hipEventDestroy(e0)
        hip.lib.hipEventDestroy(e1)
        hip.lib.hipStreamDestroy(stream)


def markdown(results, steps, warmup):
    out = ["# adanerf_render_masked: measured cost", "",
           "One session on one MI355X, library sources `%s` (`adanerf_amd.build.source_hash()`), `tools/measure_masked.py --steps %d --warmup %d`: "
           "medians of %d calls after %d warm-ups.  Workload: `bench.py`'s default (config 2's model: N 8, threshold 0.2, bf16 shading, split-fp16 "
           "sampling), RGBA8 output only, no aux maps.  wall: host clock around the call (it ends synchronised); events: HIP events on the "
           "context's stream around the call; stage columns: the call's `adanerf_stats`." % (adanerf_amd.build.source_hash(), steps, warmup, steps, warmup), ""]
    for res in results:
        w, h, n = res["width"], res["height"], res["rays"]
        out += ["## %d x %d (%d rays)" % (w, h, n), "",
                "| call | M | M / R | wall ms (min .. max) | events ms | stats total | sample_mlp | compact | shade_mlp | composite | scatter (derived) |",
                "|---|---|---|---|---|---|---|---|---|---|---|"]
        line = "| %s | %d | %.1f %% | %.3f (%.3f .. %.3f) | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %s |"
        f = res["render"]
        out.append(line % ("`adanerf_render`", n, 100.0, f["wall_ms"], f["wall_min_ms"], f["wall_max_ms"], f["event_ms"], f["ms_total"], f["ms_sample_mlp"],
                           f["ms_compact"], f["ms_shade_mlp"], f["ms_composite"], "-"))
        e = res["masked_empty"]
        out.append(line % ("masked, nothing selected", 0, 0.0, e["wall_ms"], e["wall_min_ms"], e["wall_max_ms"], e["event_ms"], e["ms_total"], e["ms_sample_mlp"],
                           e["ms_compact"], e["ms_shade_mlp"], e["ms_composite"], "-"))
        for x in res["masked"]:
            out.append(line % ("masked, " + x["kind"], x["rays"], 100.0 * x["fraction"], x["wall_ms"], x["wall_min_ms"], x["wall_max_ms"], x["event_ms"],
                               x["ms_total"], x["ms_sample_mlp"], x["ms_compact"], x["ms_shade_mlp"], x["ms_composite"], "%.4f" % x["scatter_ms"]))
        d, q = res["derived"], res["quality"]
        out += ["",
                "- fixed cost (M -> 0): %.4f ms wall, of which %.4f ms between the events (mask to bit words, bit words to list, the 4-byte read-back and its "
                "synchronisation)." % (d["fixed_cost_wall_ms"], d["list_kernels_event_ms"]),
                "- slope per ray, (wall at 100 %% - fixed cost) / R: random %.4f us, clustered %.4f us; the full frame costs %.4f us per ray." % (
                    d["slope_per_ray_us"]["random"], d["slope_per_ray_us"]["clustered"], d["full_per_ray_us"]),
                "- the 100 %% case over `adanerf_render`: random %+.3f ms (%+.1f %%), clustered %+.3f ms (%+.1f %%); its frame equals `adanerf_render`'s byte for "
                "byte: %s." % (d["overhead_100pct_wall_ms"]["random"], 100.0 * d["overhead_100pct"]["random"], d["overhead_100pct_wall_ms"]["clustered"],
                               100.0 * d["overhead_100pct"]["clustered"], d["same_bytes_at_100pct"]),
                "- holes of the warp on this path: %d of %d pixels without the fill (%.2f %%), %d with it (%.2f %%); re-rendered: holes %d, unsourced %d." % (
                    q["holes_unfilled"], n, 100.0 * q["holes_unfilled"] / n, q["holes_filled"], 100.0 * q["holes_filled"] / n, q["rerendered_holes"],
                    q["rerendered_unsourced"]),
                "- 8-bit PSNR against the frame rendered at the destination pose: warped %.2f dB, warped + holes %.2f dB, warped + unsourced %.2f dB." % (
                    q["psnr_warped"], q["psnr_warped_holes"], q["psnr_warped_unsourced"]), ""]
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
