"""Times frames under a sample cap (adanerf_set_sample_cap) beside uncapped frames of the same context, for
profiles/sample_cap_measured.md: bench.py's config 2 (800 x 800, N 8, threshold 0.2) and config 5 (1920 x 1080 NDC), bf16 shading,
split-fp16 sampling, camera at the view-cell centre.

Per workload, median (min .. max) of --steps synchronous adanerf_render calls after --warmup, from the library's own per-stage events
(adanerf_stats): the frame with no cap; with a cap at N (nothing launched); with a cap just above the frame's mean (the cap's launches
run, little or nothing is trimmed); with caps at 0.9 / 0.75 / 0.5 of the uncapped mean.  Per trimming cap also: the threshold t* it chose, the samples
kept, the 8-bit PSNR of the capped frame against the uncapped one, and the same frame rendered with no cap and the threshold set by hand
to t* (adanerf_set_selection) -- byte-identical, so the difference of the two times is the price of deciding on the device.  The cap's
launches are inside the `compact` stage.

--plain-only measures the uncapped frame alone through entry points every earlier build has; with --root DIR the package and bench.py are
taken from DIR (another checkout, e.g. the parent commit): the two builds' uncapped frames, alternated in one session, give the
run-to-run spread.  --trace-frames K renders K frames under --trace-cap and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the per-kernel times.

    python tools/measure_sample_cap.py [--workloads config2 config5_ndc] [--steps 30] [--warmup 5] [--out FILE.md] [--json FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ("ms_total", "ms_sample_mlp", "ms_compact", "ms_shade_mlp", "ms_composite")


def psnr8(a, b):
    mse = float(np.mean((a[:, :3].astype(np.float64) / 255.0 - b[:, :3].astype(np.float64) / 255.0) ** 2))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def timed(r, out8, rgb, steps, warmup):
    """per stage: median, min, max over `steps` synchronous frames; the last frame's sample total"""
    recs = []
    for _ in range(warmup + steps):
        st = r.render(out8, rgb, stats=True)
        recs.append({k: float(getattr(st, k)) for k in STAGES})
    recs = recs[warmup:]
    return {k: dict(med=statistics.median(x[k] for x in recs), min=min(x[k] for x in recs), max=max(x[k] for x in recs)) for k in STAGES}, int(st.total_samples)


def measure(adanerf_amd, model_dir, w, h, n_max, steps, warmup, plain_only):
    n = w * h
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(model_dir, w, h)) as r:
        r.set_camera(np.array(list(r.info.view_cell_center), np.float32), np.eye(3, dtype=np.float32))
        out8, rgb = r.empty((n, 4), np.uint8), r.empty((n, 3), np.float32)
        plain, total = timed(r, out8, rgb, steps, warmup)
        res = dict(width=w, height=h, rays=n, n_max=n_max, threshold=float(r.info.threshold), plain=plain, plain_samples=total, rows=[])
        if plain_only:
            return res
        base = out8.numpy()
        mean = total / float(n)
        res["plain_again"] = None
        settings = [("cap at N (nothing launched)", float(n_max)), ("cap just above the mean (launched)", min(float(n_max) - 0.01, mean * 1.05))]
        settings += [("cap %.2f x mean" % f, max(1.0, f * mean)) for f in (0.9, 0.75, 0.5)]
        for label, cap in settings:
            r.set_sample_cap(cap)
            t, kept = timed(r, out8, rgb, steps, warmup)
            rep = r.sample_cap_report()
            frame = out8.numpy()
            row = dict(label=label, cap=cap, times=t, kept=kept, tstar=float(rep.threshold_max), batches_trimmed=int(rep.batches_trimmed),
                       psnr=psnr8(frame, base), fraction=kept / float(total))
            assert kept <= int(np.floor(np.float64(np.float32(cap)) * n)), (label, kept)
            r.set_sample_cap(0)
            if rep.batches_trimmed:      # the same frame with the threshold set by hand: the price of deciding on the device
                r.set_selection(None, float(rep.threshold_max))
                row["by_hand"], hand_kept = timed(r, out8, rgb, steps, warmup)
                assert hand_kept == kept and np.array_equal(out8.numpy(), frame), "the frame at the threshold t* differs from the capped frame"
                r.set_selection(None, res["threshold"])
            res["rows"].append(row)
        res["plain_again"], _ = timed(r, out8, rgb, steps, warmup)      # the uncapped frame once more: the spread inside this process
        assert np.array_equal(out8.numpy(), base), "the frame with the cap removed differs from the first uncapped frame"
        return res


def cell(x):
    return "%.4f (%.4f .. %.4f)" % (x["med"], x["min"], x["max"])


def markdown(results, steps, warmup, source_hash):
    out = ["One session on one MI355X, library sources `%s` (`adanerf_amd.build.source_hash()`), `tools/measure_sample_cap.py --steps %d --warmup %d`: "
           "ms, median (min .. max) of %d synchronous `adanerf_render` calls after %d warm-ups, from the library's per-stage events.  bf16 shading, "
           "split-fp16 sampling, RGBA8 and fp32 colour outputs, camera at the view-cell centre." % (source_hash, steps, warmup, steps, warmup), ""]
    for name, res in results:
        out += ["## %s: %d x %d, N %d, threshold %g (%d rays, %.3f samples per ray uncapped)" %
                (name, res["width"], res["height"], res["n_max"], res["threshold"], res["rays"], res["plain_samples"] / float(res["rays"])), "",
                "| frame | cap | t* | samples kept | of uncapped | PSNR vs uncapped | frame | sampling | compact (cap inside) | shading | compositing | frame, threshold t* by hand | its compact | cap - by hand |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]

        def line(label, cap, tstar, kept, frac, psnr, t, hand):
            return "| %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
                label, cap, tstar, kept, frac, psnr, cell(t["ms_total"]), cell(t["ms_sample_mlp"]), cell(t["ms_compact"]), cell(t["ms_shade_mlp"]),
                cell(t["ms_composite"]), cell(hand["ms_total"]) if hand else "-", cell(hand["ms_compact"]) if hand else "-",
                "%+.4f" % (t["ms_total"]["med"] - hand["ms_total"]["med"]) if hand else "-")
        out.append(line("no cap", "-", "-", str(res["plain_samples"]), "1.000", "-", res["plain"], None))
        for x in res["rows"]:
            out.append(line(x["label"], "%.3f" % x["cap"], "%.6g" % x["tstar"] if x["batches_trimmed"] else "-", str(x["kept"]), "%.3f" % x["fraction"],
                            "%.2f dB" % x["psnr"] if x["psnr"] != float("inf") else "identical", x["times"], x.get("by_hand")))
        if res.get("plain_again"):
            out.append(line("no cap, again at the end", "-", "-", str(res["plain_samples"]), "1.000", "identical", res["plain_again"], None))
        out.append("")
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workloads", nargs="+", default=["config2", "config5_ndc"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the checkout whose adanerf_amd and bench.py are used")
    ap.add_argument("--trace-frames", type=int, default=0)
    ap.add_argument("--trace-cap", type=float, default=0.0)
    ap.add_argument("--out", default=None, help="the tables as markdown")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(a.root))
    import adanerf_amd
    import bench
    adanerf_amd.build_library()
    results = []
    with tempfile.TemporaryDirectory() as td:
        for name in a.workloads:
            w, h, n_max, thr, tag = bench.WORKLOADS[name]
            d = os.path.join(td, name)
            os.makedirs(d)
            bench.build_model_dir(d, tag, n_max, thr)
            if a.trace_frames:
                with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
                    r.set_camera(np.array(list(r.info.view_cell_center), np.float32), np.eye(3, dtype=np.float32))
                    out8 = r.empty((w * h, 4), np.uint8)
                    if a.trace_cap:
                        r.set_sample_cap(a.trace_cap)
                    for _ in range(a.trace_frames):
                        st = r.render(out8, None, stats=True)
                    print("%s: %d frames under cap %g, %d samples" % (name, a.trace_frames, a.trace_cap, st.total_samples))
                continue
            results.append((name, measure(adanerf_amd, d, w, h, n_max, a.steps, a.warmup, a.plain_only)))
    if a.trace_frames:
        return
    if a.plain_only:
        for name, res in results:
            print("%s plain (%s): %s" % (name, os.path.abspath(a.root), ", ".join("%s %s" % (k, cell(res["plain"][k])) for k in STAGES)), flush=True)
    text = markdown(results, a.steps, a.warmup, adanerf_amd.build.source_hash())
    if not a.plain_only:
        print(text, flush=True)
    for path, body in ((a.out, text), (a.json, json.dumps(dict(steps=a.steps, warmup=a.warmup, source_hash=adanerf_amd.build.source_hash(), root=os.path.abspath(a.root),
                                                                results=results), indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(body + "\n")


if __name__ == "__main__":
    main()
