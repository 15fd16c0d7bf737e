"""Times adanerf_temporal_upsample (two launches, clamp on, every optional buffer) beside the renders it stands between, for
profiles/upsample_measured.md: on one context, a render at the small size w x h, the upsample call into s w x s h, a render at the native
size s w x s h, and adanerf_temporal_resolve at the native size (the stage this one is measured against).  HIP events on the context's
stream, median of --steps calls after --warmup.  The frames are real jittered renders of bench.py's default workload (config2's model)
with their own depth_map / acc_map; the history is what one cycle of s x s frames at rest left, the timed call's pose a hundredth of the view
cell away from it.  Also counted: the pixels rejected per call at rest when the history's depth is tested all the same.

    python tools/measure_upsample.py [--cases 400x400x2 960x540x2 640x360x3] [--steps 30] [--warmup 5] [--out FILE.json]
                                     [--rest-case classroom_n8_thr02]     also: that test case's model (tests/golden) at 24 x 16 and 48 x 32, s 2,
                                                                          rejected per call at rest with the history's depth tested
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
from measure_reproject import Hip       # noqa: E402

# per OUTPUT pixel: colour 12, depth 4, count 1, rgba8 4, mask 1 written; gathered from the history: the nearest tap's depth 4 and count 1
# and four colour taps of 12 that neighbouring pixels share (about 12 from memory).  Per RENDER pixel: colour 12 + depth_map 4 + acc_map 4
# read, zp 4 written and read.
BYTES_OUT, BYTES_HISTORY, BYTES_RENDER = 12 + 4 + 1 + 4 + 1, 12 + 4 + 1, 12 + 4 + 4 + 4 + 4


def rest_with_depth(r, s, pos, rot, calls):
    """rejected per call at rest from a cut with the history's depth passed on every call (the hosts pass none at rest): the render at the
    next offset of the cycle, then the device call itself on buffers of the tool's own"""
    n, N = r.info.width * r.info.height, r.info.width * r.info.height * s * s
    sets = [(r.empty((N, 3), np.float32), r.empty((N,), np.float32), r.empty((N,), np.uint8)) for _ in range(2)]
    grid = r.subpixel_grid(s)
    rejected = []
    r.set_camera(pos, rot)
    for k in range(calls):
        r.reset_upsample()
        r._tu["k"] = k
        r.render_upsampled()      # leaves the frame jittered by grid[k % s^2] in _o_rgb / _rp_depth / _rp_acc
        dx, dy = grid[k % len(grid)]
        hist = sets[(k + 1) % 2] if k else (None, None, None)
        out = sets[k % 2]
        rejected.append(r.temporal_upsample_device(s, r._o_rgb, r._rp_depth, r._rp_acc, dx, dy, pos, rot, hist[0], hist[1], hist[2], pos if k else None,
                                                   rot if k else None, out[0], out[1], out[2]))
    for st in sets:
        for b in st:
            b.free()
    return rejected


def measure(model_dir, w, h, s, steps, warmup, hip):
    stream, e0, e1 = hip.make("hipStreamCreate"), hip.make("hipEventCreate"), hip.make("hipEventCreate")
    W, H = s * w, s * h
    n, N = w * h, W * H
    try:
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(model_dir, w, h)) as r:
            r.set_stream(stream.value)
            pos = np.array(list(r.info.view_cell_center), np.float32)
            rot = np.eye(3, dtype=np.float32)
            step = (np.float32(0.01) * np.array(list(r.info.view_cell_size), np.float32)).astype(np.float32)
            med = lambda stats, f: statistics.median(getattr(x, f) for x in stats)
            # ---- the small render and the upsample
            r.enable_temporal_upsample(scale=s)
            r.set_camera(pos, rot)
            small, rest = [], []
            for k in range(max(s * s, 4)):      # whole cycles at rest: every output pixel has had its own sample
                out = r.render_upsampled()
                small.append(out[4])
                rest.append(out[3])
            r.set_camera(pos + step, rot)
            moved = r.render_upsampled()      # leaves the jittered frame in _o_rgb / _rp_depth / _rp_acc, and flips the history
            dx, dy = r._tu["offsets"][(r._tu["k"] - 1) % (s * s)]
            hist = r._tu_sets[1 - r._tu_hist[0]]      # the set render_upsampled read last, at pos
            out = (r.empty((N, 3), np.float32), r.empty((N,), np.float32), r.empty((N,), np.uint8), r.empty((N, 4), np.uint8), r.empty((N,), np.uint8))
            call = lambda **kw: r.temporal_upsample_device(s, r._o_rgb, r._rp_depth, r._rp_acc, dx, dy, pos + step, rot, hist[0], hist[1], hist[2], pos, rot,
                                                           out[0], out[1], out[2], out[3], out[4], **kw)
            ms = [hip.timed(stream, e0, e1, lambda: call(rejected=False)) for _ in range(warmup + steps)][warmup:]
            counted = call()
            same = np.array_equal(out[0].numpy().view(np.uint8), r._tu_sets[r._tu_hist[0]][0].numpy().view(np.uint8))      # what render_upsampled wrote
            no_depth = lambda: r.temporal_upsample_device(s, r._o_rgb, r._rp_depth, r._rp_acc, dx, dy, pos + step, rot, hist[0], None, hist[2], pos, rot,
                                                          out[0], out[1], out[2], out[3], out[4], rejected=False)
            ms_b = [hip.timed(stream, e0, e1, no_depth) for _ in range(warmup + steps)][warmup:]      # pass B alone: no history depth, no pass A
            with_depth = rest_with_depth(r, s, pos, rot, 2 * s * s + 1)
            for b in out:
                b.free()
            # ---- the native render and the temporal resolve at the native size, same context
            r.set_frame_size(W, H)
            r.enable_temporal(grid=2)
            r.set_camera(pos, rot)
            native = [r.render_temporal()[4] for _ in range(4)]
            r.set_camera(pos + step, rot)
            ta_rejected = r.render_temporal()[3]
            th = r._ta_sets[1 - r._ta_hist[0]]
            tout = (r.empty((N, 3), np.float32), r.empty((N,), np.float32), r.empty((N,), np.uint8), r.empty((N, 4), np.uint8), r.empty((N,), np.uint8))
            resolve = lambda: r.temporal_resolve_device(r._o_rgb, r._rp_depth, r._rp_acc, pos + step, rot, th[0], th[1], th[2], pos, rot, tout[0], tout[1],
                                                        tout[2], tout[3], tout[4], rejected=False)
            ms_t = [hip.timed(stream, e0, e1, resolve) for _ in range(warmup + steps)][warmup:]
            stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
            return dict(width=w, height=h, scale=s, upsample=stat(ms), upsample_no_history_depth=stat(ms_b), temporal_resolve_native=stat(ms_t),
                        render_small_ms=med(small, "ms_total"), render_native_ms=med(native, "ms_total"), rejected_moved=counted,
                        rejected_moved_by_render_upsampled=moved[3], same_bits_as_render_upsampled=bool(same), rejected_at_rest=rest,
                        rejected_at_rest_with_history_depth=with_depth, temporal_resolve_rejected_moved=ta_rejected, output_pixels=N,
                        bytes_model=(BYTES_OUT + BYTES_HISTORY) * N + BYTES_RENDER * n)
    finally:
        hip.lib.hipEventDestroy(e0)
        hip.lib.hipEventDestroy(e1)
        hip.lib.hipStreamDestroy(stream)


def rest_case(name, sizes=((24, 16), (48, 32)), s=2, calls=9):
    """the at-rest count on a test case's model and pose: the frames tests/test_gpu_temporal.py and profiles/temporal_measured.md speak of"""
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    import adanerf_oracle as O
    from conftest import case_weights, load_case
    z, meta, sc = load_case(name)
    out = []
    with tempfile.TemporaryDirectory() as td:
        O.write_model_dir(td, sc, case_weights(meta))
        for (w, h) in sizes:
            with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(td, w, h)) as r:
                r.enable_temporal_upsample(scale=s)
                rejected = rest_with_depth(r, s, np.asarray(z["pose"], np.float32), np.asarray(z["rot"], np.float32), calls)
            out.append(dict(case=name, width=w, height=h, scale=s, rejected_at_rest_with_history_depth=rejected))
            print("%s %dx%d -> %dx%d, history depth tested at rest, depth_tol 0.02: rejected per call %s" % (name, w, h, s * w, s * h, rejected), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", nargs="+", default=["400x400x2", "960x540x2", "640x360x3"], help="render width x height x scale")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rest-case", default=None, help="a case of tests/golden: its at-rest count at 24 x 16 and 48 x 32, s 2")
    a = ap.parse_args(argv)
    if a.steps < 20:
        ap.error("--steps: at least 20 timed calls")
    adanerf_amd.build_library()
    hip = Hip()
    _, _, n, thr, tag = bench.WORKLOADS["config2"]
    results = []
    with tempfile.TemporaryDirectory() as td:
        bench.build_model_dir(td, tag, n, thr)
        for case in a.cases:
            w, h, s = (int(v) for v in case.split("x"))
            res = measure(td, w, h, s, a.steps, a.warmup, hip)
            results.append(res)
            u, t = res["upsample"], res["temporal_resolve_native"]
            both = res["render_small_ms"] + u["median_ms"]
            print("%dx%d -> %dx%d: upsample %.4f ms (min %.4f, max %.4f; without history depth %.4f); temporal resolve at %dx%d %.4f ms, ratio %.2f; "
                  "render small %.3f ms, render native %.3f ms: small + upsample %.3f ms = %.3f of native; %.2f TB/s on the bytes model; rejected on the "
                  "move %d of %d (%.1f %%; temporal resolve at the native size: %d); at rest %s; at rest with the history's depth tested %s; same bits as "
                  "render_upsampled %s" % (
                      w, h, s * w, s * h, u["median_ms"], u["min_ms"], u["max_ms"], res["upsample_no_history_depth"]["median_ms"], s * w, s * h,
                      t["median_ms"], u["median_ms"] / t["median_ms"], res["render_small_ms"], res["render_native_ms"], both, both / res["render_native_ms"],
                      res["bytes_model"] / (u["median_ms"] * 1e-3) / 1e12, res["rejected_moved"], res["output_pixels"],
                      100.0 * res["rejected_moved"] / res["output_pixels"], res["temporal_resolve_rejected_moved"], res["rejected_at_rest"],
                      res["rejected_at_rest_with_history_depth"], res["same_bits_as_render_upsampled"]), flush=True)
    rest = rest_case(a.rest_case) if a.rest_case else []
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(steps=a.steps, warmup=a.warmup, source_hash=adanerf_amd.build.source_hash(), results=results, rest_case=rest), f, indent=1)


if __name__ == "__main__":
    main()
