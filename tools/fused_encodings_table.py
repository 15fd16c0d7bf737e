#!/usr/bin/env python3
"""The tables of profiles/fused_encodings_measured.md from the lines tests/test_gpu_fused_encodings.py writes to $ADANERF_MEASURED_LOG:

    ADANERF_MEASURED_LOG=LOG python -m pytest tests/test_gpu_fused_encodings.py -m gpu
    grep '"test": "fused_encodings' LOG > profiles/fused_encodings_measured.log
    python tools/fused_encodings_table.py profiles/fused_encodings_measured.log > TABLES.md

The note's prose stands above the tables and is kept by hand."""
import collections
import json
import sys


def main(path):
    lines = [json.loads(l) for l in open(path) if l.strip()]
    scenes = [l for l in lines if l["test"] == "fused_encodings_scene"]
    bands = [l for l in lines if l["test"] == "fused_encodings_band"]
    two = [l for l in lines if l["test"] == "fused_encodings_two_block"]
    w = print
    w("%d slot values read, %d outside their bound.\n" % (sum(l["slots"] for l in bands), sum(l["outside"] for l in bands)))
    w("## Scenes (conditions asserted on the device's own x) and what a case costs\n")
    w("| stage | case | scene | bands | largest \\|a\\| | largest revolutions | share of top-band arguments beyond 256 revolutions (x, y, z) | mixed 64-row waves | mixed 128-row tiles | contexts | seconds |")
    w("|---|---|---|---|---|---|---|---|---|---|---|")
    for l in scenes:
        w("| %s | %s | %s | %d | %.0f | %.1f | %s | %s | %s | %s | %.2f |" % (
            l["stage"], l["case"], l["scene"], l["bands"], l["max_abs_a"], l["max_rev"], ", ".join("%.3f" % v for v in l["share_beyond_256"]),
            l.get("mixed_waves", "-"), l.get("mixed_tiles", "-"), l.get("contexts", "-"), l.get("seconds", float("nan"))))
    w("\n## Per kernel class and scene (all cases and bands together)\n")
    w("Filed under the kernel that ran.  needed the widening: the largest per-band share of slots whose output is not the probe's value on the "
      "expected slot itself (E = 0 would have failed them).\n")
    w("| stage | kernel class / form | scene | sin / cos slots | outside | needed the widening (worst band) | max \\|out - sin64(a)\\| | identity slots | outside |")
    w("|---|---|---|---|---|---|---|---|---|")
    agg = collections.OrderedDict()
    for l in bands:
        a = agg.setdefault((l["stage"], l["engine"], l["scene"]), dict(t=0, to=0, tw=0.0, te=0.0, i=0, io=0))
        if l["band"] < 0:
            a["i"] += l["slots"]
            a["io"] += l["outside"]
        else:
            a["t"] += l["slots"]
            a["to"] += l["outside"]
            a["tw"] = max(a["tw"], l["needed_widening"])
            a["te"] = max(a["te"], l["max_abs_err"])
    for (st, e, s), a in agg.items():
        w("| %s | %s | %s | %d | %d | %.2e | %.2e | %d | %d |" % (st, e, s, a["t"], a["to"], a["tw"], a["te"], a["i"], a["io"]))
    w("\n## Per band: the fast form on the fixed kernels, far scene (10-4)\n")
    w("| kernel | block | band | slots | needed the widening | max \\|out - sin64(a)\\| |")
    w("|---|---|---|---|---|---|")
    for l in bands:
        if l["scene"] == "far" and l["engine"].endswith("/fast") and l["case"] in ("fixed_10_4", "fixed_8x256") and l["band"] >= 0:
            kern = "sample_mlp16_kernel (fp16)" if l["stage"] == "sampling" else "shade_mlp16x2_kernel (%s)" % l["engine"].split("/")[0]
            w("| %s | %s | %d | %d | %.2e | %.2e |" % (kern, l["block"], l["band"], l["slots"], l["needed_widening"], l["max_abs_err"]))
    w("\n## The two-block kernel against the 8-wave kernel (every comparison an equality)\n")
    w("Share of (ray, slot) values that reached the kept values through the 16-slot probes, plain and negated (beyond +-2^-10).\n")
    w("| case | scene | probes | contexts | rays | slots | kept share, the least-seen slot | kept share, mean | seconds |")
    w("|---|---|---|---|---|---|---|---|---|")
    for l in two:
        w("| %s | %s | %d | %d | %d | %d | %.3f | %.3f | %.2f |" % (l["case"], l["scene"], l["probes"], l["contexts"], l["rays"], l["slots"],
                                                                  l["kept_share_min"], l["kept_share_mean"], l["seconds"]))


if __name__ == "__main__":
    main(sys.argv[1])
