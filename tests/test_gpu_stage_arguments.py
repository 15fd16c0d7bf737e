"""The argument checks of the sixteen image-space entry points (csrc/stages.hip), as one table: for every call below the return code and
the COMPLETE adanerf_last_error text equal tests/golden/stage_arguments.json, and a caller-visible count (holes_out, rejected_out,
unfilled_out, n_flagged, mean_out) keeps its sentinel.  Every row is a call that is rejected before anything is launched; there is a
row for every fail(...) site of those entry points and of the rules they call (density_rule_fill, contrast_rule_check), and for every
entry point with more than one check a row that breaks two rules at once (labels with a `+`), which pins the check that fires first.
One site has no row: flip_prepare's "filter radius outside 1..19" cannot be reached through adanerf_flip, whose pixels_per_degree
range (10..140) keeps both radii inside it.

Where the expected values come from: never from the library under test.  The record was written by this file's own `__main__`
(`python tests/test_gpu_stage_arguments.py tests/golden/stage_arguments.json`) in a checkout of commit 80db1fb8ae50 -- the parent of
the commit that moved these entry points out of adanerf_hip.hip -- against the library built from that checkout, on an MI355X.  A
row with a NULL context records the code alone (adanerf_last_error(NULL) is the creating thread's last create error, not this call's).

Pointers are offsets into one 4 MB device allocation, 256 KB apart: no row dereferences one, and no message holds an address.
Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle")]

import adanerf_oracle as O
from conftest import GOLD, case_weights, load_case

import adanerf_amd

pytestmark = pytest.mark.gpu

RECORD = os.path.join(GOLD, "stage_arguments.json")
W, H = 16, 12
N = W * H
BIG = (2048, 1024)      # the one frame size at which scale 4 reaches temporal_upsample's 2^25 output pixels; the context's batch stays 192 rays
SLOT, SLOTS = 256 * 1024, 16
SENTINEL = -7
NAN, INF = float("nan"), float("inf")


class P:
    """slot k of the device allocation, `off` bytes in"""
    def __init__(self, k, off=0):
        self.k, self.off = k, off


class I32(list):
    """a host array of int32"""


OUT, OUT_F32, NO_CTX = "out:int32", "out:float", "no context"
POS, ROT = (0.5, -3.0, 1.25), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
BAD_POS, BAD_ROT = (0.5, NAN, 1.25), (1.0, 0.0, 0.0, 0.0, INF, 0.0, 0.0, 0.0, 1.0)

_TEMPORAL = [("cur_rgb", P(1)), ("cur_depth", P(2)), ("cur_acc", P(3)), ("cur_pos", POS), ("cur_rot", ROT), ("hist_rgb", P(4)), ("hist_depth", P(5)),
             ("hist_count", P(6)), ("prev_pos", POS), ("prev_rot", ROT), ("alpha", 0.25), ("depth_tol", 0.05), ("acc_min", 0.5), ("flags", 1),
             ("out_rgb", P(7)), ("out_depth", P(8)), ("out_count", P(9)), ("out_rgba8", P(10)), ("out_mask", P(11)), ("count", OUT)]
_RINGS = [("gaze_x", 8.0), ("gaze_y", 6.0), ("n_rings", 2), ("radius", I32([3, 6])), ("stride", I32([1, 2, 4]))]
_FILL = [("rgb", P(1)), ("depth", P(2)), ("acc", P(3)), ("rgba8", P(4)), ("count", OUT)]

# entry point -> its arguments behind the context, in order, with the values of a call that is accepted
GOOD = {
    "adanerf_accumulate": [("rgb", P(0)), ("n_rays", N), ("sum", P(1)), ("first", 1)],
    "adanerf_accumulate_masked": [("rgb", P(0)), ("mask", P(2)), ("values", 1), ("n_rays", N), ("sum", P(1)), ("first", 1)],
    "adanerf_resolve_mean": [("sum", P(0)), ("n_rays", N), ("frames", 4), ("rgba8", P(1)), ("rgb", P(2))],
    "adanerf_resolve_mean_masked": [("sum", P(0)), ("mask", P(3)), ("values", 1), ("n_rays", N), ("frames", 4), ("rgba8", P(1)), ("rgb", P(2))],
    "adanerf_present": [("src", P(0)), ("src_w", W), ("src_h", H), ("dst", P(1)), ("dst_w", 2 * W), ("dst_h", 2 * H), ("flags", 0)],
    "adanerf_reproject": [("src", P(0)), ("depth", P(1)), ("acc", P(2)), ("src_pos", POS), ("src_rot", ROT), ("dst_pos", POS), ("dst_rot", ROT), ("acc_min", 0.5),
                          ("hole", 0xFF000000), ("flags", 1), ("dst", P(3)), ("dst_depth", P(4)), ("dst_mask", P(5)), ("count", OUT)],
    "adanerf_temporal_resolve": _TEMPORAL,
    "adanerf_temporal_upsample": [("scale", 2)] + _TEMPORAL[:3] + [("cur_dx", 0.25), ("cur_dy", -0.25)] + _TEMPORAL[3:],
    "adanerf_temporal_resolve_sparse": [("mask", P(0)), ("phase_x", 3), ("phase_y", 5)] + _TEMPORAL,
    "adanerf_blend_behind": [("rgb", P(0)), ("acc", P(1)), ("behind", P(2)), ("n", N), ("out_rgb", P(3)), ("out_rgba8", P(4))],
    "adanerf_foveate_density": _RINGS + [("mask", P(0))],
    "adanerf_foveate_density_phased": _RINGS + [("phase_x", 3), ("phase_y", 5), ("mask", P(0))],
    "adanerf_fill_density": [("mask", P(0)), ("width", W), ("height", H)] + _FILL,
    "adanerf_fill_density_phased": [("mask", P(0)), ("width", W), ("height", H), ("phase_x", 3), ("phase_y", 5)] + _FILL,
    "adanerf_contrast_mask": [("rgb", P(0)), ("width", W), ("height", H), ("threshold", 0.1), ("mask", P(1)), ("count", OUT)],
    "adanerf_flip": [("test", P(0)), ("ref", P(1)), ("width", W), ("height", H), ("ppd", 0.0), ("map", P(2)), ("count", OUT_F32)],
}

TOO_MANY = 0x7fffffff // 3 + 1


def _temporal_rows(fn, out_bytes=N):
    """the checks the three temporal resolves share; out_bytes: pixels of the output"""
    rows = [(fn, lbl, kw) for lbl, kw in [
        ("no context", {NO_CTX: True}),
        ("NULL cur_rgb", dict(cur_rgb=None)), ("NULL cur_depth", dict(cur_depth=None)), ("NULL cur_acc", dict(cur_acc=None)), ("NULL out_rgb", dict(out_rgb=None)),
        ("NULL cur_pos", dict(cur_pos=None)), ("NULL cur_rot", dict(cur_rot=None)), ("NULL prev_pos", dict(prev_pos=None)), ("NULL prev_rot", dict(prev_rot=None)),
        ("cur_pos not finite", dict(cur_pos=BAD_POS)), ("cur_rot not finite", dict(cur_rot=BAD_ROT)), ("prev_pos not finite", dict(prev_pos=BAD_POS)),
        ("prev_rot not finite", dict(prev_rot=BAD_ROT)),
        ("alpha 0", dict(alpha=0.0)), ("alpha 1.5", dict(alpha=1.5)), ("alpha NaN", dict(alpha=NAN)), ("depth_tol < 0", dict(depth_tol=-1.0)),
        ("depth_tol NaN", dict(depth_tol=NAN)), ("acc_min < 0", dict(acc_min=-0.5)), ("acc_min NaN", dict(acc_min=NAN)), ("flags 2", dict(flags=2)),
        ("flags -1", dict(flags=-1)),
        ("cur_rgb misaligned", dict(cur_rgb=P(1, 2))), ("cur_depth misaligned", dict(cur_depth=P(2, 1))), ("cur_acc misaligned", dict(cur_acc=P(3, 3))),
        ("hist_rgb misaligned", dict(hist_rgb=P(4, 2))), ("hist_depth misaligned", dict(hist_depth=P(5, 2))), ("out_rgb misaligned", dict(out_rgb=P(7, 1))),
        ("out_depth misaligned", dict(out_depth=P(8, 1))), ("out_rgba8 misaligned", dict(out_rgba8=P(10, 2))),
        ("out_rgb on hist_rgb", dict(out_rgb=P(4))), ("out_rgb in cur_rgb", dict(out_rgb=P(1, 8))), ("out_depth on hist_depth", dict(out_depth=P(5, 4))),
        ("out_count on hist_count", dict(out_count=P(6, out_bytes - 1))),
        ("NULL image + NULL pose", dict(cur_depth=None, cur_pos=None)), ("NULL pose + not finite", dict(cur_rot=None, prev_pos=BAD_POS)),
        ("not finite + alpha", dict(prev_rot=BAD_ROT, alpha=2.0)), ("alpha + depth_tol + acc_min + flags", dict(alpha=0.0, depth_tol=-1.0, acc_min=-1.0, flags=4)),
        ("depth_tol + acc_min", dict(depth_tol=NAN, acc_min=-1.0)), ("acc_min + flags", dict(acc_min=-1.0, flags=2)), ("flags + misaligned", dict(flags=2, out_rgb=P(7, 2))),
        ("misaligned + overlap", dict(cur_acc=P(3, 1), out_rgb=P(4))),
        ("useNDC", dict(ctx="ndc")), ("shard_world 2", dict(ctx="shard")), ("overlap + useNDC", dict(ctx="ndc", out_rgb=P(4))),
        ("misaligned + shard_world 2", dict(ctx="shard", hist_depth=P(5, 2))), ("flags + useNDC", dict(ctx="ndc", flags=2)),
    ]]
    # without a history the previous pose is not read: the call gets as far as the next rule that is broken
    rows += [(fn, "no history: NULL prev pose, then alpha", dict(hist_rgb=None, prev_pos=None, prev_rot=None, alpha=0.0)),
             (fn, "no history: prev pose not finite, then flags", dict(hist_rgb=None, prev_pos=BAD_POS, prev_rot=BAD_ROT, flags=2))]
    return rows


def _rings_rows(fn, phased):
    rows = [(fn, lbl, kw) for lbl, kw in [
        ("no context", {NO_CTX: True}), ("NULL mask", dict(mask=None)), ("gaze NaN", dict(gaze_x=NAN)), ("gaze inf", dict(gaze_y=INF)),
        ("n_rings -1", dict(n_rings=-1)), ("n_rings 9", dict(n_rings=9)), ("NULL radius", dict(radius=None)), ("NULL stride", dict(stride=None)),
        ("radius < 0", dict(radius=I32([-1, 6]))), ("radii not ascending", dict(radius=I32([6, 6]))), ("stride 3", dict(stride=I32([1, 3, 4]))),
        ("strides decrease", dict(stride=I32([2, 1, 4]))), ("shard_world 2", dict(ctx="shard")),
        ("NULL mask + gaze", dict(mask=None, gaze_x=NAN)), ("gaze + n_rings", dict(gaze_x=INF, n_rings=9)), ("n_rings + NULL array", dict(n_rings=-1, stride=None)),
        ("radii + strides", dict(radius=I32([6, 3]), stride=I32([8, 4, 2]))), ("strides + shard_world 2", dict(ctx="shard", stride=I32([1, 5, 8]))),
    ]]
    if phased:
        rows += [(fn, lbl, kw) for lbl, kw in [
            ("phase_x -1", dict(phase_x=-1)), ("phase_y 8", dict(phase_y=8)), ("NULL array + phase", dict(radius=None, phase_x=8)),
            ("phase + radii", dict(phase_y=-1, radius=I32([6, 3])))]]
    return rows


def _fill_rows(fn, phased):
    rows = [(fn, lbl, kw) for lbl, kw in [
        ("no context", {NO_CTX: True}), ("NULL mask", dict(mask=None)), ("NULL rgb", dict(rgb=None)), ("width 0", dict(width=0)), ("height 16385", dict(height=16385)),
        ("rgb misaligned", dict(rgb=P(1, 2))), ("depth misaligned", dict(depth=P(2, 1))), ("acc misaligned", dict(acc=P(3, 3))), ("rgba8 misaligned", dict(rgba8=P(4, 2))),
        ("mask in rgb", dict(mask=P(1, 16))), ("depth on rgb", dict(depth=P(1, 4 * 3 * N - 4))), ("acc on depth", dict(acc=P(2))), ("rgba8 in acc", dict(rgba8=P(3, 4))),
        ("mask in rgba8", dict(mask=P(4, 4 * N - 1))),
        ("NULL + side", dict(rgb=None, width=0)), ("side + misaligned", dict(height=0, rgb=P(1, 2))), ("misaligned + overlap", dict(depth=P(2, 2), acc=P(2))),
    ]]
    if phased:
        rows += [(fn, lbl, kw) for lbl, kw in [
            ("phase_x 8", dict(phase_x=8)), ("phase_y -1", dict(phase_y=-1)), ("side + phase", dict(width=16385, phase_x=8)),
            ("phase + misaligned", dict(phase_y=9, rgba8=P(4, 1)))]]
    return rows


def _rows(fn, *pairs):
    return [(fn, lbl, kw) for lbl, kw in pairs]


TABLE = (
    _rows("adanerf_accumulate",
          ("no context", {NO_CTX: True}), ("NULL rgb", dict(rgb=None)), ("NULL sum", dict(sum=None)), ("n_rays -1", dict(n_rays=-1)),
          ("n_rays too many", dict(n_rays=TOO_MANY)), ("rgb misaligned", dict(rgb=P(0, 2))), ("sum misaligned", dict(sum=P(1, 1))),
          ("sum inside rgb", dict(sum=P(0, 4))), ("NULL + n_rays", dict(sum=None, n_rays=-1)), ("n_rays + misaligned", dict(n_rays=-1, rgb=P(0, 1))),
          ("misaligned + overlap", dict(rgb=P(0, 2), sum=P(0, 4))))
    + _rows("adanerf_accumulate_masked",
            ("no context", {NO_CTX: True}), ("NULL rgb", dict(rgb=None)), ("NULL sum", dict(sum=None)), ("NULL mask", dict(mask=None)), ("values 0", dict(values=0)),
            ("n_rays -1", dict(n_rays=-1)), ("n_rays too many", dict(n_rays=TOO_MANY)), ("rgb misaligned", dict(rgb=P(0, 2))), ("sum misaligned", dict(sum=P(1, 1))),
            ("sum inside rgb", dict(sum=P(0, 4))), ("mask in sum", dict(mask=P(1, 5))), ("NULL image + NULL mask", dict(rgb=None, mask=None)),
            ("values 0 + n_rays", dict(values=0, n_rays=-1)), ("n_rays + misaligned", dict(n_rays=TOO_MANY, sum=P(1, 2))),
            ("misaligned + overlap", dict(rgb=P(0, 2), sum=P(0, 4))), ("both overlaps", dict(sum=P(0, 4), mask=P(0, 9))))
    + _rows("adanerf_resolve_mean",
            ("no context", {NO_CTX: True}), ("NULL sum", dict(sum=None)), ("both outputs NULL", dict(rgba8=None, rgb=None)), ("n_rays -1", dict(n_rays=-1)),
            ("n_rays too many", dict(n_rays=TOO_MANY)), ("frames 0", dict(frames=0)), ("frames 65537", dict(frames=65537)), ("sum misaligned", dict(sum=P(0, 2))),
            ("rgba8 misaligned", dict(rgba8=P(1, 1))), ("rgb misaligned", dict(rgb=P(2, 3))), ("rgb inside sum", dict(rgb=P(0, 4))), ("rgba8 on sum", dict(rgba8=P(0))),
            ("rgba8 inside rgb", dict(rgba8=P(2, 8))), ("NULL + n_rays", dict(sum=None, n_rays=-1)), ("n_rays + frames", dict(n_rays=-1, frames=0)),
            ("frames + misaligned", dict(frames=0, rgb=P(2, 1))), ("misaligned + overlap", dict(sum=P(0, 2), rgba8=P(0, 4))))
    + _rows("adanerf_resolve_mean_masked",
            ("no context", {NO_CTX: True}), ("NULL sum", dict(sum=None)), ("both outputs NULL", dict(rgba8=None, rgb=None)), ("NULL mask", dict(mask=None)),
            ("values 0", dict(values=0)), ("n_rays -1", dict(n_rays=-1)), ("n_rays too many", dict(n_rays=TOO_MANY)), ("frames 0", dict(frames=0)),
            ("frames 65537", dict(frames=65537)), ("sum misaligned", dict(sum=P(0, 2))), ("rgba8 misaligned", dict(rgba8=P(1, 1))), ("rgb misaligned", dict(rgb=P(2, 3))),
            ("rgb inside sum", dict(rgb=P(0, 4))), ("rgba8 on sum", dict(rgba8=P(0))), ("rgba8 inside rgb", dict(rgba8=P(2, 8))), ("mask in rgb", dict(mask=P(2, 7))),
            ("mask in rgba8", dict(mask=P(1, 4 * N - 1))), ("NULL sum + NULL mask", dict(sum=None, mask=None)), ("values 0 + frames", dict(values=0, frames=0)),
            ("frames + misaligned", dict(frames=0, rgb=P(2, 1))), ("misaligned + overlap", dict(sum=P(0, 2), rgba8=P(0, 4))),
            ("both overlaps", dict(rgb=P(0, 4), mask=P(1, 3))))
    + _rows("adanerf_present",
            ("no context", {NO_CTX: True}), ("NULL src", dict(src=None)), ("NULL dst", dict(dst=None)), ("src_w 0", dict(src_w=0)), ("dst_h 16385", dict(dst_h=16385)),
            ("unknown flag", dict(flags=16)), ("two filters", dict(flags=2 | 4)), ("area with linear", dict(flags=8 | 4)),
            ("area beyond 8", dict(flags=8, src_w=W, src_h=H, dst_w=1, dst_h=H)), ("src misaligned", dict(src=P(0, 2))), ("dst misaligned", dict(dst=P(1, 1))),
            ("dst inside src", dict(dst=P(0, 4 * N - 4))), ("NULL + side", dict(src=None, src_h=0)), ("side + flags", dict(dst_w=0, flags=16)),
            ("flags + area beyond 8", dict(flags=8 | 16, dst_w=1)), ("area beyond 8 + misaligned", dict(flags=8, dst_w=1, dst=P(1, 2))),
            ("misaligned + overlap", dict(src=P(0, 2), dst=P(0, 4))))
    + _rows("adanerf_reproject",
            ("no context", {NO_CTX: True}), ("NULL src", dict(src=None)), ("NULL depth", dict(depth=None)), ("NULL acc", dict(acc=None)), ("NULL dst", dict(dst=None)),
            ("NULL src_pos", dict(src_pos=None)), ("NULL src_rot", dict(src_rot=None)), ("NULL dst_pos", dict(dst_pos=None)), ("NULL dst_rot", dict(dst_rot=None)),
            ("src_pos not finite", dict(src_pos=BAD_POS)), ("src_rot not finite", dict(src_rot=BAD_ROT)), ("dst_pos not finite", dict(dst_pos=BAD_POS)),
            ("dst_rot not finite", dict(dst_rot=BAD_ROT)), ("acc_min < 0", dict(acc_min=-0.5)), ("acc_min NaN", dict(acc_min=NAN)), ("flags 2", dict(flags=2)),
            ("src misaligned", dict(src=P(0, 2))), ("dst misaligned", dict(dst=P(3, 1))), ("dst inside src", dict(dst=P(0, 4 * N - 4))),
            ("useNDC", dict(ctx="ndc")), ("shard_world 2", dict(ctx="shard")),
            ("NULL image + NULL pose", dict(acc=None, dst_rot=None)), ("NULL pose + not finite", dict(src_pos=None, dst_pos=BAD_POS)),
            ("not finite + acc_min", dict(dst_rot=BAD_ROT, acc_min=-1.0)), ("acc_min + flags", dict(acc_min=NAN, flags=2)),
            ("flags + misaligned", dict(flags=2, dst=P(3, 2))), ("misaligned + overlap", dict(src=P(0, 2), dst=P(0, 4))),
            ("overlap + useNDC", dict(ctx="ndc", dst=P(0))), ("misaligned + shard_world 2", dict(ctx="shard", src=P(0, 1))))
    + _temporal_rows("adanerf_temporal_resolve")
    + _temporal_rows("adanerf_temporal_upsample", out_bytes=4 * N)
    + _rows("adanerf_temporal_upsample",
            ("scale 0", dict(scale=0)), ("scale 5", dict(scale=5)), ("cur_dx 1.5", dict(cur_dx=1.5)), ("cur_dy NaN", dict(cur_dy=NAN)),
            ("output 2^25 pixels", dict(ctx="big", scale=4)), ("out_depth in cur_depth", dict(out_depth=P(2, 4))), ("out_depth in cur_acc", dict(out_depth=P(3, 4 * N - 4))),
            ("not finite + scale", dict(cur_pos=BAD_POS, scale=0)), ("scale + offset", dict(scale=9, cur_dx=-2.0)), ("offset + alpha", dict(cur_dy=INF, alpha=0.0)),
            ("misaligned + 2^25", dict(ctx="big", scale=4, out_depth=P(8, 2))), ("2^25 + overlap", dict(ctx="big", scale=4, out_rgb=P(4))))
    + _temporal_rows("adanerf_temporal_resolve_sparse")
    + _rows("adanerf_temporal_resolve_sparse",
            ("NULL mask", dict(mask=None)), ("NULL out_count", dict(out_count=None)), ("history without count", dict(hist_count=None)), ("phase_x -1", dict(phase_x=-1)),
            ("phase_y 8", dict(phase_y=8)), ("mask in out_rgb", dict(mask=P(7, 8))), ("mask in out_depth", dict(mask=P(8, 4 * N - 1))), ("mask on out_count", dict(mask=P(9))),
            ("mask in out_rgba8", dict(mask=P(10, 5))), ("out_mask in mask", dict(out_mask=P(0, N - 1))),
            ("NULL mask + NULL image", dict(mask=None, cur_rgb=None)), ("NULL image + NULL out_count", dict(out_rgb=None, out_count=None)),
            ("NULL out_count + history without count", dict(out_count=None, hist_count=None)), ("history without count + phase", dict(hist_count=None, phase_x=8)),
            ("phase + NULL pose", dict(phase_y=-1, cur_pos=None)), ("both overlaps", dict(out_rgb=P(4), mask=P(9))), ("mask overlap + useNDC", dict(ctx="ndc", mask=P(9))))
    + _rows("adanerf_blend_behind",
            ("no context", {NO_CTX: True}), ("NULL rgb", dict(rgb=None)), ("NULL acc", dict(acc=None)), ("NULL behind", dict(behind=None)),
            ("both outputs NULL", dict(out_rgb=None, out_rgba8=None)), ("n -1", dict(n=-1)), ("n too many", dict(n=TOO_MANY)), ("acc misaligned", dict(acc=P(1, 2))),
            ("out_rgba8 misaligned", dict(out_rgba8=P(4, 1))), ("out_rgb inside rgb", dict(out_rgb=P(0, 4))), ("out_rgb on acc", dict(out_rgb=P(1))),
            ("out_rgba8 on rgb", dict(out_rgba8=P(0))), ("out_rgba8 in behind", dict(out_rgba8=P(2, 8))), ("outputs overlap", dict(out_rgba8=P(3, 12 * N - 4))),
            ("NULL input + NULL outputs", dict(rgb=None, out_rgb=None, out_rgba8=None)), ("NULL outputs + n", dict(out_rgb=None, out_rgba8=None, n=-1)),
            ("n + misaligned", dict(n=-1, behind=P(2, 2))), ("misaligned + overlap", dict(rgb=P(0, 2), out_rgb=P(1))),
            ("out_rgba8 on rgb + out_rgb on acc", dict(out_rgba8=P(0), out_rgb=P(1))), ("out_rgb on behind + outputs overlap", dict(out_rgb=P(2), out_rgba8=P(2, 4))))
    + _rings_rows("adanerf_foveate_density", False)
    + _rings_rows("adanerf_foveate_density_phased", True)
    + _fill_rows("adanerf_fill_density", False)
    + _fill_rows("adanerf_fill_density_phased", True)
    + _rows("adanerf_contrast_mask",
            ("no context", {NO_CTX: True}), ("NULL rgb", dict(rgb=None)), ("NULL mask", dict(mask=None)), ("width 0", dict(width=0)), ("height 16385", dict(height=16385)),
            ("threshold NaN", dict(threshold=NAN)), ("threshold < 0", dict(threshold=-0.1)), ("threshold > 1", dict(threshold=1.5)), ("rgb misaligned", dict(rgb=P(0, 2))),
            ("mask in rgb", dict(mask=P(0, 12 * N - 1))), ("NULL + side", dict(mask=None, width=0)), ("side + threshold", dict(height=0, threshold=NAN)),
            ("threshold + misaligned", dict(threshold=2.0, rgb=P(0, 1))), ("misaligned + overlap", dict(rgb=P(0, 2), mask=P(0, 8))))
    + _rows("adanerf_flip",
            ("no context", {NO_CTX: True}), ("NULL test", dict(test=None)), ("NULL ref", dict(ref=None)), ("width 0", dict(width=0)), ("height -1", dict(height=-1)),
            ("2^31 pixels", dict(width=65536, height=32768)), ("ppd 5", dict(ppd=5.0)), ("ppd 200", dict(ppd=200.0)), ("ppd NaN", dict(ppd=NAN)),
            ("NULL + side", dict(ref=None, width=0)), ("side + ppd", dict(height=0, ppd=5.0)), ("2^31 pixels + ppd", dict(width=65536, height=32768, ppd=NAN)))
)


def row_id(row):
    return "%s: %s" % (row[0], row[1])


def _model_dir(case, parent):
    z, meta, sc = load_case(case)
    d = os.path.join(parent, case)
    os.makedirs(d, exist_ok=True)
    O.write_model_dir(d, sc, case_weights(meta))
    return d


def run_table(tmp):
    """{row id: [rc, message or None, the count behind the call or None]} of every row of TABLE, on three 16 x 12 contexts: a plain one
    (its batch 192 rays at any frame size, so that the BIG rows allocate nothing), a useNDC model's, one of two shards'"""
    plain, ndc = _model_dir("classroom_n8_thr02", tmp), _model_dir("ndc_synthetic_n8", tmp)
    got = {}
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(plain, W, H, batch_size=N)) as r_plain, \
            adanerf_amd.NeuralRenderer(adanerf_amd.Settings(ndc, W, H)) as r_ndc, \
            adanerf_amd.NeuralRenderer(adanerf_amd.Settings(plain, W, H), shard_world=2, shard_rank=0) as r_shard:
        ctxs = {"plain": r_plain, "big": r_plain, "ndc": r_ndc, "shard": r_shard}
        arena = {k: r.empty((SLOT * SLOTS,), np.uint8).ptr for k, r in ctxs.items() if k != "big"}
        arena["big"] = arena["plain"]
        for row in sorted(TABLE, key=lambda row: row[2].get("ctx") == "big"):      # the resized context's rows last
            fn, _, kw = row
            kw = dict(kw)
            kind = kw.pop("ctx", "plain")
            no_ctx = kw.pop(NO_CTX, False)
            r = ctxs[kind]
            if kind == "big" and (r.info.width, r.info.height) != BIG:
                r.set_frame_size(*BIG)
            names = [a for a, _ in GOOD[fn]]
            assert set(kw) <= set(names), (row_id(row), sorted(set(kw) - set(names)))
            args, count, keep = [], None, []
            for name, good in GOOD[fn]:
                v = kw.get(name, good)
                if isinstance(v, P):
                    v = arena[kind] + v.k * SLOT + v.off
                elif isinstance(v, I32):
                    v = (C.c_int32 * len(v))(*v)
                elif isinstance(v, tuple):
                    v = (C.c_float * len(v))(*v)
                elif v == OUT:
                    v = count = C.c_int32(SENTINEL)
                elif v == OUT_F32:
                    v = count = C.c_float(SENTINEL)
                keep.append(v)
                args.append(C.byref(v) if v is count and v is not None else v)
            rc = getattr(r.lib, fn)(None if no_ctx else r.handle, *args)
            msg = None if no_ctx else r.lib.adanerf_last_error(r.handle).decode()
            assert row_id(row) not in got, "two rows named %s" % row_id(row)
            got[row_id(row)] = [rc, msg, None if count is None else int(count.value)]
        r_plain.set_frame_size(W, H)
    return got


@pytest.fixture(scope="module")
def record():
    return json.load(open(RECORD))


def test_the_record_holds_rejections_only_and_every_row_of_the_table(record):
    rows = record["rows"]
    assert sorted(rows) == sorted(row_id(row) for row in TABLE) and len(rows) == len(TABLE)
    assert all(rc in (-1, -4) for rc, _ in rows.values()), [k for k, v in rows.items() if v[0] not in (-1, -4)]
    assert {fn for fn, _, _ in TABLE} == set(GOOD)
    for fn in GOOD:      # every entry point with more than one check: a row that breaks two rules
        assert any(f == fn and "+" in lbl for f, lbl, _ in TABLE), fn
    # every message names its entry point and nothing else's
    for k, (rc, msg) in rows.items():
        assert msg is None or msg.startswith(k.split(":")[0] + ": "), (k, msg)


def test_every_rejected_call_returns_the_recorded_code_and_text_and_leaves_the_count_alone(record, tmp_path_factory):
    adanerf_amd.build_library()
    got = run_table(str(tmp_path_factory.mktemp("stage_arguments")))
    wrong = ["%s: (%d, %r), recorded (%d, %r)" % (k, got[k][0], got[k][1], rc, msg) for k, (rc, msg) in record["rows"].items() if got[k][:2] != [rc, msg]]
    assert not wrong, "%d of %d rows differ from the record:\n%s" % (len(wrong), len(got), "\n".join(wrong))
    written = [k for k, v in got.items() if v[2] not in (None, SENTINEL)]
    assert not written, "a rejected call wrote its count: %s" % written


if __name__ == "__main__":
    import subprocess
    import tempfile
    adanerf_amd.build_library()
    with tempfile.TemporaryDirectory() as tmp:
        rows = run_table(tmp)
    assert all(v[2] in (None, SENTINEL) for v in rows.values())
    head = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    with open(sys.argv[1], "w") as f:
        json.dump({"commit": head or (sys.argv[2] if len(sys.argv) > 2 else ""), "rows": {k: v[:2] for k, v in sorted(rows.items())}}, f, indent=0)
        f.write("\n")
    print("%d rows, %d rejected" % (len(rows), sum(v[0] != 0 for v in rows.values())))
