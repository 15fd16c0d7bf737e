"""Times adanerf_reproject (clear + splat + resolve, three launches) beside a rendered frame of the same context, for
profiles/reproject_measured.md.  HIP events on the context's stream, median of --steps calls after --warmup; the frame that is warped is
a real render of bench.py's default workload (config2's model) with its own depth_map / acc_map, the destination pose a tenth of the
view cell away.

    python tools/measure_reproject.py [--sizes 800x800 1920x1080] [--steps 30] [--warmup 5] [--out FILE.json]

--gather adds, in the same session and on the same frame, adanerf_reproject_gather (two launches) at iterations 1, 2, 3, 4, 8 x depth_tol
0.02, 0.05, 0.1 beside the splat (fill on), for profiles/reproject_gather_measured.md: the median time of the call with nothing read
back, the mask-0 and mask-2 fractions, and the 8-bit PSNR against the frame rendered at the destination pose -- as warped, with the
holes re-rendered and with every unsourced pixel re-rendered (adanerf_render_masked, values 1 / 5).  --table FILE writes those rows as
a markdown table.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import adanerf_amd                      # noqa: E402
import bench                            # noqa: E402
from adanerf_amd import renderer as R   # noqa: E402


class Hip:
    """the four runtime calls an event timing needs"""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")
        for name, args in (("hipStreamCreate", [C.POINTER(C.c_void_p)]), ("hipStreamDestroy", [C.c_void_p]), ("hipEventCreate", [C.POINTER(C.c_void_p)]),
                           ("hipEventDestroy", [C.c_void_p]), ("hipEventRecord", [C.c_void_p, C.c_void_p]), ("hipEventSynchronize", [C.c_void_p]),
                           ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p])):
            getattr(self.lib, name).argtypes = args
            getattr(self.lib, name).restype = C.c_int

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: hipError %d" % (what, rc))

    def make(self, name):
        h = C.c_void_p()
        self.check(getattr(self.lib, name)(C.byref(h)), name)
        return h

    def timed(self, stream, e0, e1, fn):
        self.check(self.lib.hipEventRecord(e0, stream), "hipEventRecord")
        fn()
        self.check(self.lib.hipEventRecord(e1, stream), "hipEventRecord")
        self.check(self.lib.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = C.c_float(0)
        self.check(self.lib.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        return float(ms.value)


GATHER_ITERATIONS, GATHER_TOLS = (1, 2, 3, 4, 8), (0.02, 0.05, 0.1)


def psnr8(a, b):
    mse = float(np.mean((a[:, :3].astype(np.float64) / 255.0 - b[:, :3].astype(np.float64) / 255.0) ** 2))
    return float("inf") if mse == 0 else -10.0 * float(np.log10(mse))


def measure_gather(r, hip, stream, e0, e1, pos, rot, dst, steps, warmup):
    """the splat and every (iterations, depth_tol) of the gather on one rendered frame: rows of dict(warp, iterations, depth_tol, median_ms,
    mask0, mask2 (fractions), psnr_warped, psnr_holes, psnr_unsourced, rerendered_holes, rerendered_unsourced (fractions))"""
    n = r.info.width * r.info.height
    r.set_camera(dst, rot)
    fresh = r.render_numpy()[1].copy()      # what the destination pose really shows
    r.set_camera(pos, rot)
    r.render_numpy()                        # the frame that is warped, kept by enable_reprojection()
    out_rgb, out, mask = r.empty((n, 3), np.float32), r.empty((n, 4), np.uint8), r.empty((n,), np.uint8)
    rows = []

    def quality(row, warped, m, rerender):
        row.update(mask0=float(np.mean(m == 0)), mask2=float(np.mean(m == 2)), psnr_warped=psnr8(warped, fresh))
        for mode in ("holes", "unsourced"):
            rgba, _, _, rendered = rerender(mode)
            row["psnr_" + mode], row["rerendered_" + mode] = psnr8(rgba, fresh), rendered / float(n)
        rows.append(row)

    call = lambda: r.reproject_device(r._o_rgba, r._rp_depth, r._rp_acc, pos, rot, dst, rot, out, None, mask, fill=True, holes=False)
    ms = [hip.timed(stream, e0, e1, call) for _ in range(warmup + steps)][warmup:]
    warped, m, _ = r.reproject(dst, rot)
    quality(dict(warp="splat", iterations=None, depth_tol=None, median_ms=statistics.median(ms)), warped, m, lambda mode: r.reproject_rerender(dst, rot, mode))
    for it in GATHER_ITERATIONS:
        for tol in GATHER_TOLS:
            call = lambda: r.reproject_gather_device(r._rp_rgb, r._rp_depth, r._rp_acc, pos, rot, dst, rot, out_rgb, out, None, mask, depth_tol=tol,
                                                     iterations=it, holes=False)
            ms = [hip.timed(stream, e0, e1, call) for _ in range(warmup + steps)][warmup:]
            _, warped, m, _ = r.reproject_gather(dst, rot, iterations=it, depth_tol=tol)
            quality(dict(warp="gather", iterations=it, depth_tol=tol, median_ms=statistics.median(ms)), warped, m,
                    lambda mode: r.reproject_gather_rerender(dst, rot, mode, iterations=it, depth_tol=tol))
    r.set_camera(pos, rot)
    return rows


def gather_table(results):
    lines = []
    for res in results:
        lines += ["", "### %d x %d" % (res["width"], res["height"]), "",
                  "| warp | iterations | depth_tol | call, ms | mask 0 | mask 2 | PSNR warped | PSNR, holes re-rendered (px) | PSNR, unsourced re-rendered (px) |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for x in res["gather"]:
            lines.append("| %s | %s | %s | %.4f | %.2f %% | %.2f %% | %.2f dB | %.2f dB (%.1f %%) | %.2f dB (%.1f %%) |" % (
                x["warp"], x["iterations"] or "-", x["depth_tol"] or "-", x["median_ms"], 100 * x["mask0"], 100 * x["mask2"], x["psnr_warped"], x["psnr_holes"],
                100 * x["rerendered_holes"], x["psnr_unsourced"], 100 * x["rerendered_unsourced"]))
    return "\n".join(lines) + "\n"


def measure(model_dir, w, h, steps, warmup, hip, gather=False):
    stream, e0, e1 = hip.make("hipStreamCreate"), hip.make("hipEventCreate"), hip.make("hipEventCreate")
    try:
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(model_dir, w, h)) as r:
            r.set_stream(stream.value)
            r.enable_reprojection()
            pos = np.array(list(r.info.view_cell_center), np.float32)
            rot = np.eye(3, dtype=np.float32)
            r.set_camera(pos, rot)
            frames = [r.render_numpy()[2] for _ in range(warmup + steps)][warmup:]
            dst = (pos + np.float32(0.1) * np.array(list(r.info.view_cell_size), np.float32)).astype(np.float32)
            n = w * h
            out, depth, mask = r.empty((n, 4), np.uint8), r.empty((n,), np.float32), r.empty((n,), np.uint8)
            rows = {}
            for tag, kw in (("colour only", dict()), ("colour + depth + mask", dict(dst_depth=depth, dst_mask=mask))):
                call = lambda: r.reproject_device(r._o_rgba, r._rp_depth, r._rp_acc, pos, rot, dst, rot, out, fill=True, holes=False, **kw)
                ms = [hip.timed(stream, e0, e1, call) for _ in range(warmup + steps)][warmup:]
                rows[tag] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
            holes = r.reproject_device(r._o_rgba, r._rp_depth, r._rp_acc, pos, rot, dst, rot, out, fill=True)
            bare = r.reproject_device(r._o_rgba, r._rp_depth, r._rp_acc, pos, rot, dst, rot, out, fill=False)
            med = lambda f: statistics.median(getattr(s, f) for s in frames)
            extra = dict(gather=measure_gather(r, hip, stream, e0, e1, pos, rot, dst, steps, warmup)) if gather else {}
            # bytes the three launches move: z-buffer cleared (8), depth + acc read (8), one 8-byte atomic per landed pixel (<= 8), z-buffer read (8),
            # colour gathered and written (4 + 4); + 5 with depth and mask
            return dict(width=w, height=h, reproject=rows, holes_filled=holes, holes_unfilled=bare, bytes_colour_only=40 * n, bytes_all_outputs=45 * n,
                        render=dict(ms_total=med("ms_total"), ms_compact=med("ms_compact"), ms_composite=med("ms_composite"),
                                    ms_sample_mlp=med("ms_sample_mlp"), ms_shade_mlp=med("ms_shade_mlp")), **extra)
    finally:
        hip.lib.hipEventDestroy(e0)
        hip.lib.hipEventDestroy(e1)
        hip.lib.hipStreamDestroy(stream)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", nargs="+", default=["800x800", "1920x1080"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gather", action="store_true", help="also adanerf_reproject_gather over its two dials, with quality against the destination pose's render")
    ap.add_argument("--table", default=None, help="with --gather: write the rows as a markdown table")
    a = ap.parse_args(argv)
    adanerf_amd.build_library()
    hip = Hip()
    _, _, n, thr, tag = bench.WORKLOADS["config2"]
    results = []
    with tempfile.TemporaryDirectory() as td:
        bench.build_model_dir(td, tag, n, thr)
        for size in a.sizes:
            w, h = (int(v) for v in size.split("x"))
            res = measure(td, w, h, a.steps, a.warmup, hip, a.gather)
            results.append(res)
            full = res["reproject"]["colour + depth + mask"]["median_ms"]
            print("%dx%d: reproject %.4f ms (colour only %.4f), rendered frame %.3f ms (compaction %.3f + composite %.3f), ratio %.4f, holes %d (%d unfilled)" % (
                w, h, full, res["reproject"]["colour only"]["median_ms"], res["render"]["ms_total"], res["render"]["ms_compact"],
                res["render"]["ms_composite"], full / res["render"]["ms_total"], res["holes_filled"], res["holes_unfilled"]), flush=True)
            for x in res.get("gather", []):
                print("  %-6s it %-4s tol %-4s %.4f ms  mask0 %.4f mask2 %.4f  PSNR %.2f / holes %.2f (%.3f) / unsourced %.2f (%.3f)" % (
                    x["warp"], x["iterations"], x["depth_tol"], x["median_ms"], x["mask0"], x["mask2"], x["psnr_warped"], x["psnr_holes"], x["rerendered_holes"],
                    x["psnr_unsourced"], x["rerendered_unsourced"]), flush=True)
    if a.gather and a.table:
        os.makedirs(os.path.dirname(os.path.abspath(a.table)), exist_ok=True)
        with open(a.table, "w") as f:
            f.write("source hash %s, %d calls after %d warm-ups\n" % (adanerf_amd.build.source_hash(), a.steps, a.warmup) + gather_table(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(steps=a.steps, warmup=a.warmup, source_hash=adanerf_amd.build.source_hash(), results=results), f, indent=1)


if __name__ == "__main__":
    main()
