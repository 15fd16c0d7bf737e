"""Times foveated density over time beside the fill-only foveated frame and adanerf_render of the same build in the same process, and
scores what it buys, for profiles/foveated_temporal_measured.md: bench.py's default workload (config 2's model: N 8, threshold 0.2, bf16
shading, split-fp16 sampling) at 800 x 800 with 120:1,300:2,4 and at 1920 x 1080 with 200:1,500:2,4, the gaze at the frame centre.

Per size, median of --steps calls after --warmup, each both as the wall time on the host around work that ends synchronised and as HIP
events on the context's stream:
  calls    adanerf_foveate_density_phased; adanerf_fill_density_phased (fp32 colour, depth, acc; no counter); adanerf_temporal_resolve_sparse
           with the history's depth (passes A and B) and without it (pass B alone), on a moved pose; adanerf_temporal_resolve on the same
           images.  Per-kernel times come from a kernel trace of this tool (--steps small), not from here.
  frames   adanerf_render; the fill-only foveated frame (masked render + adanerf_fill_density, what render_foveated enqueues); the
           foveated temporal frame (phased mask, masked render, phased fill, sparse resolve with its counter read back, what
           render_foveated_temporal enqueues), at rest and with the pose moved every frame.
  quality  PSNR of the fp32 frame against adanerf_render's at rest after 1, 4, 16 and 64 frames of render_foveated_temporal from a cut,
           and at the last pose of a lateral path (--path-frames frames, a step of --path-step of the view cell per frame), each beside
           the fill-only frame's PSNR.

    python tools/measure_foveated_temporal.py [--sizes 800x800 1920x1080] [--steps 20] [--warmup 5] [--out FILE.md] [--json FILE.json]
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

SETTINGS = {(800, 800): "120:1,300:2,4", (1920, 1080): "200:1,500:2,4"}


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def measure(model_dir, w, h, spec, steps, warmup, path_frames, path_step, hip):
    stream, e0, e1 = hip.make("hipStreamCreate"), hip.make("hipEventCreate"), hip.make("hipEventCreate")
    n = w * h
    med = statistics.median
    try:
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(model_dir, w, h)) as r:
            r.set_stream(stream.value)
            pos0, rot = np.array(list(r.info.view_cell_center), np.float32), np.eye(3, dtype=np.float32)
            size = np.array(list(r.info.view_cell_size), np.float32)
            r.set_camera(pos0, rot)
            gaze = (0.5 * w, 0.5 * h)
            rings = R.parse_fovea_density(spec)

            def timed(fn):
                """fn enqueues (or runs) the work; the wall clock stops after a synchronisation"""
                wall, ev = [], []
                for _ in range(warmup + steps):
                    t0 = time.perf_counter()
                    ev.append(hip.timed(stream, e0, e1, fn))      # ends in hipEventSynchronize of the event behind the work
                    wall.append((time.perf_counter() - t0) * 1e3)
                wall, ev = wall[warmup:], ev[warmup:]
                return dict(wall_ms=med(wall), wall_min_ms=min(wall), wall_max_ms=max(wall), event_ms=med(ev))

            # ---- quality first: the hosts' own paths, numpy results
            full = r.render_numpy()[0].copy()
            r.foveate_density(gaze, rings)
            fill_only = r.render_foveated()[0].copy()
            r.enable_foveated_temporal()
            at_rest, rejected = {}, []
            for k in range(64):
                out = r.render_foveated_temporal()
                rejected.append(out[3])
                if k + 1 in (1, 4, 16, 64):
                    at_rest[k + 1] = psnr(out[0], full)
            poses = [(pos0 + np.float32(path_step * k) * size * np.float32([1, 1, 0])).astype(np.float32) for k in range(path_frames)]
            r.set_camera(poses[-1], rot)
            full_last = r.render_numpy()[0].copy()
            fill_last = r.render_foveated()[0].copy()
            r.reset_foveated_temporal()
            path_rejected = []
            for p in poses:
                r.set_camera(p, rot)
                out = r.render_foveated_temporal()
                path_rejected.append(out[3])
            quality = dict(fill_only=psnr(fill_only, full), at_rest={str(k): v for k, v in at_rest.items()}, rejected_at_rest=rejected[:3],
                           path_frames=path_frames, path_step=path_step, path_resolved=psnr(out[0], full_last), path_fill_only=psnr(fill_last, full_last),
                           path_rejected_fraction=[v / float(n) for v in path_rejected])

            # ---- the calls: the images render_foveated_temporal left (a filled frame, two history sets)
            r.set_camera(pos0, rot)
            out8, rgb = r._o_rgba, r._o_rgb
            dmask, depth, acc = r._ft_dmask, r._rp_depth, r._rp_acc
            side = r._ft_hist[0]
            hist, dst = r._ft_sets[side], r._ft_sets[1 - side]
            prev = r._ft_hist[1:]
            moved = (pos0 + np.float32(path_step) * size * np.float32([1, 1, 0])).astype(np.float32)
            phase = R.density_phase(37)
            mask_t = timed(lambda: r._check(r.foveate_density_phased_device(gaze, rings, phase, dmask)))
            assert np.array_equal(dmask.numpy(), R.density_mask_phased(w, h, gaze, rings, phase)), "device mask differs from the host mask"
            rendered = int(np.count_nonzero(dmask.numpy() == 0))
            r.render_masked(dmask, 1, None, rgb)
            fill_t = timed(lambda: r._check(r.fill_density_phased_device(dmask, w, h, phase, rgb, depth, acc, None, count=False)[0]))
            sparse = lambda hd: r.temporal_resolve_sparse_device(dmask, phase, rgb, depth, acc, moved, rot, hist[0], hd, hist[2], prev[0], prev[1], dst[0],  # noqa: E731
                                                                 dst[1], dst[2], r._ft_rgba, r._ft_mask, rejected=False)
            ab_t = timed(lambda: sparse(hist[1]))
            b_t = timed(lambda: sparse(None))
            plain_t = timed(lambda: r.temporal_resolve_device(rgb, depth, acc, moved, rot, hist[0], hist[1], hist[2], prev[0], prev[1], dst[0], dst[1], dst[2],
                                                              r._ft_rgba, r._ft_mask, rejected=False))

            # ---- the frames
            full_t = timed(lambda: r.render(out8, rgb, stats=True))
            fd_mask = r._fd_mask

            def fill_only_frame():
                r.render_masked(fd_mask, 1, rgba8=out8, rgb=rgb)
                r._check(r.fill_density_device(fd_mask, w, h, rgb, None, None, out8, count=False)[0])
            fill_frame_t = timed(fill_only_frame)
            state = dict(k=0, side=side, prev=prev)

            def temporal_frame(pose):
                ph = R.density_phase(state["k"])
                state["k"] += 1
                r._check(r.foveate_density_phased_device(gaze, rings, ph, dmask))
                r.render_masked(dmask, 1, None, rgb)
                r._check(r.fill_density_phased_device(dmask, w, h, ph, rgb, depth, acc, None, count=False)[0])
                hs, ds = r._ft_sets[state["side"]], r._ft_sets[1 - state["side"]]
                rest = np.array_equal(state["prev"][0], pose)
                r.temporal_resolve_sparse_device(dmask, ph, rgb, depth, acc, pose, rot, hs[0], None if rest else hs[1], hs[2], state["prev"][0], state["prev"][1],
                                                 ds[0], ds[1], ds[2], r._ft_rgba, r._ft_mask)
                state["side"], state["prev"] = 1 - state["side"], (pose, rot)
            rest_t = timed(lambda: temporal_frame(pos0))
            walk = iter([(pos0 + np.float32(path_step * (k % 16)) * size * np.float32([1, 1, 0])).astype(np.float32) for k in range(1, warmup + steps + 2)])
            move_t = timed(lambda: temporal_frame(next(walk)))
            return dict(width=w, height=h, rays=n, spec=spec, rendered=rendered, phase=list(phase), mask=mask_t, fill=fill_t, resolve_ab=ab_t, resolve_b=b_t, temporal_resolve=plain_t,
                        render=full_t, fill_only_frame=fill_frame_t, temporal_frame_at_rest=rest_t, temporal_frame_moving=move_t, quality=quality)
    finally:
        hip.lib.hipEventDestroy(e0)
        hip.lib.hipEventDestroy(e1)
        hip.lib.hipStreamDestroy(stream)


def markdown(results, steps, warmup):
    out = ["One session on one MI355X, library sources `%s` (`adanerf_amd.build.source_hash()`), `tools/measure_foveated_temporal.py --steps %d --warmup %d`: "
           "medians of %d calls after %d warm-ups.  Workload: `bench.py`'s default (config 2's model: N 8, threshold 0.2, bf16 shading, split-fp16 "
           "sampling), gaze at the frame centre.  Every time cell: wall ms median (min .. max) / events ms -- wall: host clock around the work, "
           "which ends synchronised; events: HIP events on the context's stream around it." % (adanerf_amd.build.source_hash(), steps, warmup, steps, warmup), ""]
    t = lambda x: "%.4f (%.4f .. %.4f) / %.4f" % (x["wall_ms"], x["wall_min_ms"], x["wall_max_ms"], x["event_ms"])      # noqa: E731
    for res in results:
        q = res["quality"]
        out += ["## %d x %d, `%s` (%d of %d rays at phase (%d, %d))" % (res["width"], res["height"], res["spec"], res["rendered"], res["rays"], res["phase"][0], res["phase"][1]), "",
                "| call | time |", "|---|---|",
                "| `adanerf_foveate_density_phased` | %s |" % t(res["mask"]),
                "| `adanerf_fill_density_phased` (fp32 colour, depth, acc) | %s |" % t(res["fill"]),
                "| `adanerf_temporal_resolve_sparse`, history depth tested (passes A + B) | %s |" % t(res["resolve_ab"]),
                "| `adanerf_temporal_resolve_sparse`, no history depth (pass B alone) | %s |" % t(res["resolve_b"]),
                "| `adanerf_temporal_resolve` on the same images | %s |" % t(res["temporal_resolve"]), "",
                "| frame | time | of `adanerf_render` |", "|---|---|---|"]
        for name, key in (("`adanerf_render`", "render"), ("fill-only foveated frame (`render_foveated`'s calls)", "fill_only_frame"),
                          ("foveated temporal frame at rest (`render_foveated_temporal`'s calls)", "temporal_frame_at_rest"),
                          ("foveated temporal frame, the pose moving", "temporal_frame_moving")):
            out.append("| %s | %s | %.3f |" % (name, t(res[key]), res[key]["wall_ms"] / res["render"]["wall_ms"]))
        out += ["", "| PSNR against `adanerf_render`'s fp32 frame | dB |", "|---|---|", "| fill only | %.2f |" % q["fill_only"]]
        out += ["| at rest, after %s frames from a cut | %.2f |" % (k, q["at_rest"][k]) for k in ("1", "4", "16", "64")]
        out += ["| lateral path (%d frames, %g of the view cell per frame), last pose: resolved | %.2f |" % (q["path_frames"], q["path_step"], q["path_resolved"]),
                "| the same pose, fill only | %.2f |" % q["path_fill_only"], "",
                "Rejected per frame at rest: %s.  Rejected fraction along the path: %s." % (
                    q["rejected_at_rest"], ", ".join("%.3f" % v for v in q["path_rejected_fraction"])), ""]
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", nargs="+", default=["800x800", "1920x1080"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--path-frames", type=int, default=8)
    ap.add_argument("--path-step", type=float, default=0.01)
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
            results.append(measure(td, w, h, SETTINGS.get((w, h), "120:1,300:2,4"), a.steps, a.warmup, a.path_frames, a.path_step, hip))
    text = markdown(results, a.steps, a.warmup)
    print(text, flush=True)
    for path, body in ((a.out, text), (a.json, json.dumps(dict(steps=a.steps, warmup=a.warmup, source_hash=adanerf_amd.build.source_hash(), results=results), indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(body + "\n")


if __name__ == "__main__":
    main()
