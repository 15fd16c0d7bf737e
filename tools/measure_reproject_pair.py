"""Times adanerf_reproject_pair (clear + splat of both sources + resolve, three launches) beside two adanerf_reproject calls on the same
two frames, and scores what the two warps show between two rendered frames, for profiles/reproject_pair_measured.md.  The method is
tools/measure_reproject.py's: HIP events on the context's stream around the calls with holes_out NULL, median of --steps after --warmup;
the frames are real renders of bench.py's default workload (config2's model) with their own depth_map / acc_map.

    python tools/measure_reproject_pair.py [--sizes 800x800 1920x1080] [--steps 30] [--warmup 5] [--stride 3] [--out FILE.md]

Quality: the camera walks `stride` equal steps from the view-cell centre to a pose a tenth of the view-cell size away (the distance of
profiles/reproject_measured.md).  The first and the last pose are rendered; every pose in between is shown (a) as the first frame warped
by adanerf_reproject, what --reproject K shows, and (b) as adanerf_reproject_pair of both, what --interpolate K shows, each with and
without its holes re-rendered (adanerf_render_masked, values 1), and scored against the frame rendered at that pose: fp32 PSNR for the
pair, 8-bit PSNR for both.  Reads nothing outside the repository.
"""
import argparse
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
from measure_reproject import Hip, psnr8   # noqa: E402


def psnr32(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return float("inf") if mse == 0 else -10.0 * float(np.log10(mse))


def measure(model_dir, w, h, steps, warmup, stride, hip):
    stream, e0, e1 = hip.make("hipStreamCreate"), hip.make("hipEventCreate"), hip.make("hipEventCreate")
    try:
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(model_dir, w, h)) as r:
            r.set_stream(stream.value)
            n = w * h
            pos = np.array(list(r.info.view_cell_center), np.float32)
            rot = np.eye(3, dtype=np.float32)
            end = (pos + np.float32(0.1) * np.array(list(r.info.view_cell_size), np.float32)).astype(np.float32)
            path = [(pos + np.float32(k / float(stride)) * (end - pos)).astype(np.float32) for k in range(stride + 1)]
            fresh = []
            for p in path[1:-1]:      # what the poses in between really show
                r.set_camera(p, rot)
                rgb, rgba, _ = r.render_numpy()
                fresh.append((rgb.copy(), rgba.copy()))
            b8 = r.empty((n, 4), np.uint8)      # the last pose's 8-bit frame, for the second of the two single warps that are timed
            r.set_camera(path[-1], rot)
            r.render(b8, None)
            # the one-source warp's frame: render_numpy at the first pose, kept by enable_reprojection()
            r.enable_reprojection()
            r.set_camera(path[0], rot)
            r.render_numpy()
            a8 = r._o_rgba
            # the two keyframes
            r.enable_interpolation()
            for p in (path[0], path[-1]):
                r.set_camera(p, rot)
                r.render_keyframe()
            (ka, pa, ra), (kb, pb, rb) = r._ip_keys
            A, B = r._ip_set(ka), r._ip_set(kb)
            out8, out8b, mask, maskb = r.empty((n, 4), np.uint8), r.empty((n, 4), np.uint8), r.empty((n,), np.uint8), r.empty((n,), np.uint8)
            dst = path[1]
            two = lambda: (r.reproject_device(a8, A[1], A[2], pa, ra, dst, rot, out8, None, mask, fill=True, holes=False),
                           r.reproject_device(b8, B[1], B[2], pb, rb, dst, rot, out8b, None, maskb, fill=True, holes=False))
            one = lambda: r.reproject_device(a8, A[1], A[2], pa, ra, dst, rot, out8, None, mask, fill=True, holes=False)
            pair = lambda: r.reproject_pair_device(A[0], A[1], A[2], pa, ra, B[0], B[1], B[2], pb, rb, dst, rot, r._ip_wrgb, r._ip_rgba, None, r._ip_mask,
                                                   r._ip_source, weight_b=0.5, fill=True, holes=False)
            bare = lambda: r.reproject_pair_device(A[0], A[1], A[2], pa, ra, B[0], B[1], B[2], pb, rb, dst, rot, r._ip_wrgb, None, None, None, None,
                                                   weight_b=0.5, fill=True, holes=False)
            times = {}
            for tag, call in (("one adanerf_reproject (colour + mask)", one), ("two adanerf_reproject (colour + mask each)", two),
                              ("adanerf_reproject_pair (fp32 colour, 8-bit colour, mask, source)", pair), ("adanerf_reproject_pair (fp32 colour only)", bare)):
                ms = [hip.timed(stream, e0, e1, call) for _ in range(warmup + steps)][warmup:]
                times[tag] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
            rows = []
            for p, (f_rgb, f_rgba) in zip(path[1:-1], fresh):
                row = dict(weight_b=adanerf_amd.renderer.pair_weight(p, pa, pb))
                w8, m1, holes1 = r.reproject(p, rot)
                _, _, bare1 = r.reproject(p, rot, fill=False)
                row.update(splat_holes=holes1 / float(n), splat_unfilled=bare1 / float(n), splat_filled=float(np.mean(m1 == 2)), splat_psnr8=psnr8(w8, f_rgba))
                rr8, _, _, rer = r.reproject_rerender(p, rot, "holes")
                row.update(splat_rr_psnr8=psnr8(rr8, f_rgba), splat_rerendered=rer / float(n))
                rgb, rgba, m2, src, holes2 = r.interpolate(p, rot)
                _, _, _, _, bare2 = r.interpolate(p, rot, fill=False)
                row.update(pair_holes=holes2 / float(n), pair_unfilled=bare2 / float(n), pair_filled=float(np.mean(m2 == 2)), pair_blended=float(np.mean(src == 3)),
                           pair_from_a=float(np.mean((src == 1) & (m2 == 1))), pair_from_b=float(np.mean((src == 2) & (m2 == 1))),
                           pair_psnr8=psnr8(rgba, f_rgba), pair_psnr32=psnr32(rgb, f_rgb))
                rr_rgb, rr_rgba, _, _, _, rer = r.interpolate_rerender(p, rot, "holes")
                row.update(pair_rr_psnr8=psnr8(rr_rgba, f_rgba), pair_rr_psnr32=psnr32(rr_rgb, f_rgb), pair_rerendered=rer / float(n))
                rows.append(row)
            return dict(width=w, height=h, times=times, rows=rows)
    finally:
        hip.lib.hipEventDestroy(e0)
        hip.lib.hipEventDestroy(e1)
        hip.lib.hipStreamDestroy(stream)


def report(results, steps, warmup, stride):
    lines = ["source hash %s, %d calls after %d warm-ups, stride %d" % (adanerf_amd.build.source_hash(), steps, warmup, stride), ""]
    for res in results:
        lines += ["### %d x %d" % (res["width"], res["height"]), "", "| call | median, ms | min | max |", "|---|---|---|---|"]
        for tag, t in res["times"].items():
            lines.append("| %s | %.4f | %.4f | %.4f |" % (tag, t["median_ms"], t["min_ms"], t["max_ms"]))
        lines += ["", "| pose | weight_b | warp | holes, no fill | holes | filled (mask 2) | blended / from A / from B | PSNR as shown (8-bit) | PSNR, holes re-rendered (px) |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for k, x in enumerate(res["rows"]):
            lines.append("| %d of %d | - | splat of A | %.2f %% | %.2f %% | %.2f %% | - | %.2f dB | %.2f dB (%.2f %%) |" % (
                k + 1, stride, 100 * x["splat_unfilled"], 100 * x["splat_holes"], 100 * x["splat_filled"], x["splat_psnr8"], x["splat_rr_psnr8"], 100 * x["splat_rerendered"]))
            lines.append("| %d of %d | %.4f | pair of A, B | %.2f %% | %.2f %% | %.2f %% | %.1f / %.1f / %.1f %% | %.2f dB (fp32 %.2f) | %.2f dB (fp32 %.2f) (%.2f %%) |" % (
                k + 1, stride, x["weight_b"], 100 * x["pair_unfilled"], 100 * x["pair_holes"], 100 * x["pair_filled"], 100 * x["pair_blended"], 100 * x["pair_from_a"],
                100 * x["pair_from_b"], x["pair_psnr8"], x["pair_psnr32"], x["pair_rr_psnr8"], x["pair_rr_psnr32"], 100 * x["pair_rerendered"]))
        lines.append("")
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", nargs="+", default=["800x800", "1920x1080"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stride", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the tables as markdown here")
    a = ap.parse_args(argv)
    adanerf_amd.build_library()
    hip = Hip()
    _, _, n, thr, tag = bench.WORKLOADS["config2"]
    results = []
    with tempfile.TemporaryDirectory() as td:
        bench.build_model_dir(td, tag, n, thr)
        for size in a.sizes:
            w, h = (int(v) for v in size.split("x"))
            results.append(measure(td, w, h, a.steps, a.warmup, a.stride, hip))
            print(report(results[-1:], a.steps, a.warmup, a.stride), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report(results, a.steps, a.warmup, a.stride))


if __name__ == "__main__":
    main()
