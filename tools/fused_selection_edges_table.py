"""profiles/fused_selection_edges_measured.md from the records tests/test_gpu_fused_selection_edges.py leaves in $ADANERF_MEASURED_LOG:
    ADANERF_MEASURED_LOG=LOG python -m pytest tests/test_gpu_fused_selection_edges.py -m gpu
    python tools/fused_selection_edges_table.py LOG > profiles/fused_selection_edges_measured.md"""
import datetime
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adanerf_amd import build as B


def main(path):
    recs = [json.loads(l) for l in open(path) if l.startswith("{")]
    pick = lambda name: [r for r in recs if r["test"] == name]
    pct = lambda v: "%.1f" % (100.0 * v)
    out = ["# Classes the fused selection met on the device", "",
           "`tests/test_gpu_fused_selection_edges.py` on one MI355X, %s, library sources `%s`." % (datetime.date.today().isoformat(), B.source_hash()),
           "Every comparison in that file is an equality and every one held; these are the numbers of rays and 32-ray blocks it held on.", "",
           "## Engines on exact data (stage rows against the predicted rows)", "",
           "| model | mode | rays | saturated | behind the open overflow gate | distinct rows | rows that differ |", "|---|---|---|---|---|---|---|"]
    for r in pick("fused_selection_edges_engine"):
        out.append("| %s | %s | %d | %d | %d | %d | %d |" % (r["model"], r["mode"], r["rays"], r["saturated"], r["overflow_open"], r["distinct_rows"], r["rows_differ"]))
    out += ["", "## Classes per model / engine / (N, thr)", "",
            "Shares are saturated rays of the class over all rays of the frame, in per cent; blocks are 32 consecutive rays (one wave's) that hold",
            "a ray of the class and a ray outside it.  tie: more values reach the cut than the budget; max tie: a fallback ray whose maximum repeats.", "",
            "| model | engine | rays | N | thr | kind | saturated % | tie % | fallback % | == thr % | max tie % | tie blocks | fallback blocks | max-tie blocks | non-finite rays |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in pick("fused_selection_edges_classes"):
        out.append("| %s | %s | %d | %d | %g | %s | %s | %s | %s | %s | %s | %d | %d | %d | %d |" % (
            r["model"], r["engine"], r["rays"], r["n"], r["thr"], r["kind"], pct(r["saturated"] / r["rays"]), pct(r["tie"]), pct(r["fallback"]), pct(r["at_thr"]),
            pct(r["max_tie"]), r["tie_blocks"], r["fallback_blocks"], r["max_tie_blocks"], r["nonfinite"]))
    out += ["", "## Guarded mode (97 x 61)", "",
            "| model | N | thr | band | largest difference seen | rays the rule calls undecided | tie rays | rays re-evaluated | audited | violations | audit mismatches |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in pick("fused_selection_edges_guarded"):
        out.append("| %s | %d | %g | %.4f | %.4f | %d | %d | %d | %d | %d | %d |" % (r["model"], r["n"], r["thr"], r["guard_eps"], r["guard_max_seen"], r["undecided"],
                                                                                r["ties"], r["rays_refined"], r["audited"], r["violations"], r["audit_mismatch"]))
    out += ["", "Pixels of the guarded frame that differ from the split engine's (unrefined rays outside the saturated set keep the fp16 engine's values):", "",
            "| model | N | thr | rays with the split engine's values by construction | pixels that differ |", "|---|---|---|---|---|"]
    for r in pick("fused_selection_edges_guarded_frame"):
        out.append("| %s | %d | %g | %d | %d |" % (r["model"], r["n"], r["thr"], r["exact_rays"], r["pixels_differ"]))
    print("\n".join(out))


if __name__ == "__main__":
    main(sys.argv[1])
