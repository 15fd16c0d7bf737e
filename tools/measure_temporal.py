"""Times adanerf_temporal_resolve (one launch, clamp on, every optional buffer) beside a rendered frame of the same context, for
profiles/temporal_measured.md.  HIP events on the context's stream, median of --steps calls after --warmup.  The frames that are resolved
are real jittered renders of bench.py's default workload (config2's model) with their own depth_map / acc_map; the history is what the
resolve of the frames before left, the current pose a hundredth of the view cell away from the history's.

    python tools/measure_temporal.py [--sizes 800x800 1920x1080] [--steps 30] [--warmup 5] [--out FILE.json]
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

# per pixel: current colour 12 + depth_map 4 + acc_map 4 read; colour 12, depth 4, count 1, rgba8 4, mask 1 written; gathered from the
# history: the nearest tap's depth 4 and count 1, and four colour taps of 12 that neighbouring pixels share (about 12 from memory)
BYTES_FIXED, BYTES_HISTORY = (12 + 4 + 4) + (12 + 4 + 1 + 4 + 1), 12 + 4 + 1


def prepare(r, stream, pos, rot, step):
    """a history at pos and a jittered frame at pos + step: everything one timed call reads"""
    r.set_stream(stream.value)
    r.enable_temporal(grid=2)
    stats = []
    for k in range(4):      # one cycle of offsets at rest: the history's counts reach 4 where nothing is rejected
        r.set_camera(pos, rot)
        stats.append(r.render_temporal()[4])
    r.set_camera(pos + step, rot)
    rejected = r.render_temporal()[3]      # leaves the jittered frame in _o_rgb / _rp_depth / _rp_acc, and flips the history
    return stats, rejected


def measure(model_dir, w, h, steps, warmup, hip):
    stream, e0, e1 = hip.make("hipStreamCreate"), hip.make("hipEventCreate"), hip.make("hipEventCreate")
    try:
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(model_dir, w, h)) as r:
            n = w * h
            pos = np.array(list(r.info.view_cell_center), np.float32)
            rot = np.eye(3, dtype=np.float32)
            step = (np.float32(0.01) * np.array(list(r.info.view_cell_size), np.float32)).astype(np.float32)
            frames, rejected = prepare(r, stream, pos, rot, step)
            # the history of the timed call is the set render_temporal read last (the one not written last), at pos
            hist = r._ta_sets[1 - r._ta_hist[0]]
            out = (r.empty((n, 3), np.float32), r.empty((n,), np.float32), r.empty((n,), np.uint8), r.empty((n, 4), np.uint8), r.empty((n,), np.uint8))
            call = lambda **kw: r.temporal_resolve_device(r._o_rgb, r._rp_depth, r._rp_acc, pos + step, rot, hist[0], hist[1], hist[2], pos, rot,
                                                          out[0], out[1], out[2], out[3], out[4], **kw)
            ms = [hip.timed(stream, e0, e1, lambda: call(rejected=False)) for _ in range(warmup + steps)][warmup:]
            counted = call()
            same = np.array_equal(out[0].numpy().view(np.uint8), r._ta_sets[r._ta_hist[0]][0].numpy().view(np.uint8))      # what render_temporal wrote
            med = lambda f: statistics.median(getattr(s, f) for s in frames)
            return dict(width=w, height=h, resolve=dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms)), rejected=counted,
                        rejected_by_render_temporal=rejected, same_bits_as_render_temporal=bool(same),
                        bytes_model=(BYTES_FIXED + BYTES_HISTORY) * n, bytes_fixed=BYTES_FIXED * n,
                        render=dict(ms_total=med("ms_total"), ms_compact=med("ms_compact"), ms_composite=med("ms_composite"),
                                    ms_sample_mlp=med("ms_sample_mlp"), ms_shade_mlp=med("ms_shade_mlp")))
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
    a = ap.parse_args(argv)
    if a.steps < 20:
        ap.error("--steps: at least 20 timed calls")
    adanerf_amd.build_library()
    hip = Hip()
    _, _, n, thr, tag = bench.WORKLOADS["config2"]
    results = []
    with tempfile.TemporaryDirectory() as td:
        bench.build_model_dir(td, tag, n, thr)
        for size in a.sizes:
            w, h = (int(v) for v in size.split("x"))
            res = measure(td, w, h, a.steps, a.warmup, hip)
            results.append(res)
            t = res["resolve"]
            print("%dx%d: temporal resolve %.4f ms (min %.4f, max %.4f); %.2f TB/s on %d B/pixel; rendered frame %.3f ms (compaction %.3f + composite %.3f), "
                  "ratio %.4f; rejected %d of %d; same bits as render_temporal %s" % (
                      w, h, t["median_ms"], t["min_ms"], t["max_ms"], res["bytes_model"] / (t["median_ms"] * 1e-3) / 1e12, BYTES_FIXED + BYTES_HISTORY,
                      res["render"]["ms_total"], res["render"]["ms_compact"], res["render"]["ms_composite"], t["median_ms"] / res["render"]["ms_total"],
                      res["rejected"], w * h, res["same_bits_as_render_temporal"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(steps=a.steps, warmup=a.warmup, source_hash=adanerf_amd.build.source_hash(), results=results), f, indent=1)


if __name__ == "__main__":
    main()
