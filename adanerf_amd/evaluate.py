"""Image evaluation over a DONeRF-style dataset directory with the MI355X renderer -- the counterpart of the
reference's ``src/evaluate.py`` "images" evaluation (``generate_data`` :164-342: render every test view, MSE /
PSNR against the ground-truth PNG, mean samples per ray) for an exported model directory.  ``--metrics psnr flip`` adds the
reference's second default metric (``metrics = ["flip", "psnr"]`` :613-615): the mean FLIP error of ``generate_flip_data``
(:120-145 over ``src/util/flip_loss.py``), computed on the GPU by ``adanerf_flip`` from the frame that is still in device memory.

    python -m adanerf_amd.evaluate <model_dir> <dataset_dir> [--set test] [--out DIR] [--video out.y4m] [--precision bf16]
                                   [--metrics psnr flip] [--sweep-thresholds T ...] [--sweep-samples N ...] [--sweep-scales S ...]
                                   [--reproject-stride K [--reproject-warp splat|gather] [--rerender holes|unsourced]] [--supersample S] [--present-filter nearest|linear|area]
                                   [--fovea-density R:S[,R:S...],S [--fovea-temporal ALPHA] [--fovea-temporal-still K]] [--supersample-contrast T]
                                   [--sweep-sample-caps C ...] [--interpolate-stride K [--rerender holes|unsourced]]

``--sweep-sample-caps`` renders the set once per sample cap on one context (``NeuralRenderer.set_sample_cap``: a hard bound on the mean
samples per ray of every frame, met on the device by raising the threshold): the quality a frame-time guarantee costs; the summary's
``sweep`` entries carry ``sample_cap`` and ``mean_cap_threshold``.

``--sweep-thresholds`` / ``--sweep-samples`` render the set once per (N, threshold) of their cross product on ONE context
(``NeuralRenderer.set_selection``: an AdaNeRF network is trained once and rendered at any sample budget) -- the two axes of a quality
table; the summary gains ``sweep``, ``--out DIR`` writes into ``DIR/n<N>_t<threshold>/``.  ``--sweep-scales`` is the third axis, the
resolution: the set is rendered at ``round(w S) x round(h S)`` on the same context (``NeuralRenderer.set_frame_size``), presented to the
dataset's ``w x h`` on the GPU (``adanerf_present``, the viewer's blit) and scored from that 8-bit image / 255; sub-directories gain
``_s<scale>``.

``--reproject-stride K`` renders the poses with ``i % K == 0`` and warps the others from the nearest rendered pose before them
(``adanerf_reproject``, holes filled from their neighbours): what a host that renders every K-th frame shows in between, scored against
the same ground truth.  ``--rerender holes|unsourced`` scores every warped frame once more with its holes (unsourced: the filled pixels too)
rendered at its own pose (``adanerf_render_masked``).  ``--reproject-warp gather`` makes the warped frames with ``adanerf_reproject_gather``
(``--reproject-iterations N``, ``--reproject-tol T``: its two dials) instead of the splat.

``--interpolate-stride K`` renders the poses with ``i % K == 0`` and the last one as keyframes and makes every other pose from the
keyframe before it AND the keyframe after it (``adanerf_reproject_pair``, weight from ``adanerf_host_pair_weight``, fill on): what a host
that knows its path, or shows its frames K late, shows in between.  ``--rerender`` applies to those frames as it does to warped ones.

``--supersample S`` makes every image the mean of S x S renders at the sub-pixel offsets of ``adanerf_host_subpixel_grid``, accumulated
and resolved on the GPU (``NeuralRenderer.render_supersampled``) and scored from the fp32 mean: anti-aliasing in time, against the
dataset's anti-aliased ground truth.  ``--present-filter area`` makes the ``--sweep-scales`` presentation an exact area filter
(``ADANERF_PRESENT_AREA``): the only sensible choice for scales above 1, where the default rule decimates.

``--supersample-contrast T`` (with ``--supersample S``, S >= 2) spends the S x S renders only where the frame has edges
(``NeuralRenderer.render_supersampled_adaptive``: one render at the pixel centres, ``adanerf_contrast_mask`` on it, the sub-pixel renders of
the flagged pixels alone through ``adanerf_render_masked``); the summary gains ``mean_refined_fraction``.

``--fovea-density SPEC`` scores, beside every full frame, the same pose rendered at a foveated ray density around a gaze at the frame
centre (``NeuralRenderer.render_foveated``: the lattice of ``adanerf_foveate_density`` rendered, the pixels in between rebuilt by
``adanerf_fill_density``), on the same context.  ``--fovea-temporal ALPHA`` adds, beside that fill-only frame, the same pose through
``NeuralRenderer.render_foveated_temporal`` (the lattice at the next phase of its 64-phase cycle, resolved against a history by
``adanerf_temporal_resolve_sparse``), the set in order as one sequence; ``--fovea-temporal-still K`` scores per pose the frame after K
such frames at rest from a cut instead.

Dataset layout (src/datasets.py:146-213, 361-365, 480-542): ``dataset_info.json`` (``resolution``,
``camera_angle_x``, ``view_cell_center``, ``view_cell_size`` ...), ``transforms_<set>.json`` with
``frames[i].file_path`` ("./test/00000") and ``frames[i].transform_matrix`` (4x4 camera-to-world; pose =
[:3, 3], rotation = [:3, :3]), images ``<file_path>.png``.
"""
import argparse
import itertools
import json
import math
import os
import sys
from typing import List, Optional

import numpy as np

from .png import read_png, write_png
from .renderer import GATHER_DEPTH_TOL, GATHER_ITERATIONS, PRESENT_FILTERS, RERENDER_VALUES, SUPERSAMPLE_MAX, NeuralRenderer, Settings, parse_fovea, parse_fovea_density


def load_dataset(dataset_dir: str, set_name: str = "test"):
    with open(os.path.join(dataset_dir, "dataset_info.json")) as f:
        info = json.load(f)
    with open(os.path.join(dataset_dir, "transforms_%s.json" % set_name)) as f:
        tr = json.load(f)
    w, h = int(info["resolution"][0]), int(info["resolution"][1])
    frames = []
    for fr in tr["frames"]:
        m = np.array(fr["transform_matrix"], dtype=np.float32)
        rel = fr["file_path"][2:] if fr["file_path"].startswith("./") else fr["file_path"]   # datasets.py:362
        frames.append(dict(pose=m[:3, 3].copy(), rot=m[:3, :3].copy(), image=os.path.join(dataset_dir, rel + ".png")))
    return dict(w=w, h=h, fov=float(info["camera_angle_x"]), info=info), frames


class Y4mWriter:
    """Uncompressed YUV4MPEG2 (4:4:4, BT.601 full range) -- the headless counterpart of the reference's
    ``imageio.mimwrite(... .mp4, fps=30)`` (src/evaluate.py:289-292); no codec library exists in this image, and any
    player / ffmpeg reads .y4m."""

    def __init__(self, path: str, w: int, h: int, fps: int = 30):
        self.f = open(path, "wb")
        self.f.write(("YUV4MPEG2 W%d H%d F%d:1 Ip A1:1 C444 XCOLORRANGE=FULL\n" % (w, h, fps)).encode())
        self.w, self.h = w, h

    def add(self, rgb8: np.ndarray):
        """rgb8: uint8 [h, w, 3]"""
        c = rgb8.astype(np.float32)
        y = 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]
        u = -0.168736 * c[..., 0] - 0.331264 * c[..., 1] + 0.5 * c[..., 2] + 128.0
        v = 0.5 * c[..., 0] - 0.418688 * c[..., 1] - 0.081312 * c[..., 2] + 128.0
        self.f.write(b"FRAME\n")
        for p in (y, u, v):
            self.f.write(np.clip(np.rint(p), 0, 255).astype(np.uint8).tobytes())

    def close(self):
        self.f.close()


def psnr_from_mse(mse: float) -> float:
    """src/evaluate.py:49-54: 10 log10(1 / mse), mse over all 3*h*w values."""
    return float("inf") if mse == 0 else 10.0 * math.log10(1.0 / mse)


def sweep_dir_name(num_samples: int, threshold: float, scale: Optional[float] = None) -> str:
    """Sub-directory of --out for one setting of a sweep: n<N>_t<threshold>, the threshold as %g prints it (n8_t0.1, n128_t0); with
    --sweep-scales n<N>_t<threshold>_s<scale> (n8_t0.1_s0.5)."""
    return "n%d_t%g" % (num_samples, threshold) + ("" if scale is None else "_s%g" % scale)


def scaled_size(w: int, h: int, scale: float):
    """The render size of one --sweep-scales entry: round(w S) x round(h S), at least 1 x 1."""
    return max(1, int(round(w * scale))), max(1, int(round(h * scale)))


def evaluate(model_dir: str, dataset_dir: str, set_name: str = "test", out_dir: Optional[str] = None,
             precision: str = "bf16", batch_size: int = -1, max_frames: int = 0, quiet: bool = False,
             video: Optional[str] = None, fps: int = 30, metrics=("psnr",), fovea=None, sweep_thresholds=None, sweep_samples=None, reproject_stride=None,
             supersample=None, present_filter=None, temporal=None, temporal_still=None, temporal_upsample=None, temporal_upsample_frames=None,
             rerender=None, fovea_density=None, reproject_warp="splat", reproject_iterations=None, reproject_tol=None, sweep_sample_caps=None,
             interpolate_stride=None, fovea_temporal=None, fovea_temporal_still=None, supersample_contrast=None, sweep_scales=None):
    """metrics: "psnr" (always reported where a ground-truth image exists) and / or "flip": each record gains ``flip``, the summary
    ``mean_flip``, and with out_dir the error map is written as an 8-bit greyscale ``%05d_flip.png``.

    sweep_thresholds / sweep_samples (lists; either may be None = the model's own value): the set is rendered once per (N, threshold) of
    their cross product, N outermost, all on the one context.  The summary is then ``{"frames": n, "sweep": [...]}`` with one
    ``{num_samples, threshold, mean_psnr, mean_mse, mean_samples_per_ray, mean_ms[, mean_flip]}`` per setting (what a plain run of a
    model with that setting reports), the records of all settings follow each other and carry ``num_samples`` / ``threshold``, and
    out_dir gets one sub-directory per setting (sweep_dir_name).

    sweep_scales (list or None): innermost axis of the same cross product.  Each setting renders at scaled_size(w, h, S), presents the
    frame to w x h on the device and scores THAT image (uint8 / 255, also at S = 1: the entries of one table are measured alike);
    samples_per_ray counts per rendered ray; entries and records carry ``scale``; frames written to out_dir / video are the presented ones.

    reproject_stride (K >= 1 or None): the poses with i % K == 0 are rendered, every other pose is the nearest rendered frame before it
    warped to that pose on the device (NeuralRenderer.reproject, fill on) and scored from the 8-bit result / 255.  Records gain ``warped``
    and, for a warped frame, ``hole_fraction`` (pixels nothing reached, of w h) in place of samples_per_ray / ms; the summary gains
    ``mean_psnr_rendered``, ``mean_psnr_warped``, ``mean_hole_fraction`` and, with "flip", ``mean_flip_rendered`` / ``mean_flip_warped``;
    mean_samples_per_ray / mean_ms are those of the rendered frames.  At the dataset's resolution only (not with sweep_scales).
    rerender ("holes", "unsourced" or None; needs reproject_stride): every warped frame is scored a second time with its holes (unsourced: the
    pixels filled from a neighbour too) rendered at its own pose (NeuralRenderer.reproject_rerender).  Warped records gain
    ``psnr_rerendered`` / ``mse_rerendered`` and ``rerendered_fraction`` (pixels rendered, of w h), the summary
    ``mean_psnr_warped_rerendered`` and ``mean_rerendered_fraction``; out_dir gets ``%05d_rerendered.png``.  Every other key is that of a run
    without the option.
    reproject_warp ("splat", the default, or "gather"; gather needs reproject_stride): the warped frames come from
    NeuralRenderer.reproject_gather (adanerf_reproject_gather; reproject_iterations / reproject_tol: its two dials, None = the renderer's
    defaults) and rerender uses reproject_gather_rerender.  Warped records carry ``warp``; the summary keys are unchanged.

    interpolate_stride (K >= 1 or None): the poses with i % K == 0, and the last pose, are rendered as keyframes
    (NeuralRenderer.render_keyframe); every other pose is made from the keyframe before it and the keyframe after it
    (NeuralRenderer.interpolate: adanerf_reproject_pair, the weight from pair_weight, fill on) and scored from the fp32 result.  Records
    gain ``interpolated`` and, for an interpolated frame, ``hole_fraction`` and ``blended_fraction`` (pixels both keyframes agreed on, of
    w h) in place of samples_per_ray / ms; the summary gains ``mean_psnr_rendered``, ``mean_psnr_interpolated``, ``mean_hole_fraction``,
    ``mean_blended_fraction`` and, with "flip", ``mean_flip_rendered`` / ``mean_flip_interpolated``.  With rerender every interpolated
    frame is scored a second time with its holes rendered at its own pose (NeuralRenderer.interpolate_rerender): ``psnr_rerendered`` /
    ``mse_rerendered`` / ``rerendered_fraction`` in the records, ``mean_psnr_interpolated_rerendered`` / ``mean_rerendered_fraction`` in
    the summary.  Not with reproject_stride or any other frame-to-frame option, the sweeps or fovea_density.

    supersample (S in 1..8 or None): every image is the mean of S x S renders at the offsets of the regular sub-pixel grid
    (NeuralRenderer.render_supersampled), scored from the fp32 mean; ms is the sum over the S x S renders, samples_per_ray is per rendered
    frame; records and summary carry ``supersample``.  Not together with reproject_stride (the mean has no depth map to warp by).

    supersample_contrast (T in [0, 1] or None; needs supersample >= 2): adaptive supersampling -- every image is one render at the pixel
    centres whose edge pixels (a neighbour differs by more than T in some channel's display value) are replaced by the mean of their S x S
    sub-pixel renders (NeuralRenderer.render_supersampled_adaptive).  ms is the sum over all passes, samples_per_ray is the centre
    frame's; records gain ``refined_fraction`` (pixels refined, of w h), the summary ``mean_refined_fraction``.

    present_filter (None, "nearest", "linear" or "area"): the filter of the sweep_scales presentation (NeuralRenderer.present); None is the
    viewer's rule, which decimates a frame rendered above the dataset's size -- "area" averages it.

    temporal (ALPHA in (0, 1] or None): temporal anti-aliasing beside the plain frames.  The set is walked in order as ONE sequence: after
    a pose's plain render the same pose is rendered once more at the next offset of the 2 x 2 sub-pixel cycle and resolved against the
    history of the poses before it (NeuralRenderer.render_temporal, clamp on, the default depth tolerance), and that fp32 frame is scored
    too.  Records gain ``psnr_temporal`` / ``mse_temporal``, ``rejected_fraction`` (pixels whose history was dropped, of w h; 1 on the
    first pose) and, with "flip", ``flip_temporal``; the summary ``mean_psnr_temporal``, ``mean_rejected_fraction`` and
    ``mean_flip_temporal``; out_dir gets ``%05d_temporal.png``.  The plain keys are those of a run without the option.
    temporal_still (K >= 1 or None): per pose instead, the frame after K resolves at rest from an empty history (what a viewer shows K
    frames after the camera stopped there); ALPHA is ``temporal`` or, without it, 0.1; the summary carries ``temporal_still``.
    Neither goes with reproject_stride, supersample or sweep_scales.

    temporal_upsample (S in 1..4 or None): temporal upsampling beside the plain frames.  The context renders at the dataset's size / S, which
    must divide (ValueError otherwise).  Per pose the plain frame is the un-jittered small render shown at the dataset's size by
    NeuralRenderer.present's linear filter (scored from that 8-bit image / 255); then, from an empty history and at rest, K =
    temporal_upsample_frames (default S x S) frames are rendered at the offsets of the S x S cycle and resolved at the dataset's size
    (NeuralRenderer.render_upsampled, clamp on, default alpha and tolerance), and the last fp32 frame is scored.  Records gain
    ``psnr_upsampled`` / ``mse_upsampled``, ``rejected_fraction`` (of the last call, of w h), ``temporal_upsample`` and, with "flip",
    ``flip_upsampled``; the summary ``mean_psnr_upsampled``, ``mean_rejected_fraction``, ``mean_flip_upsampled``, ``temporal_upsample``
    and ``temporal_upsample_frames``; out_dir gets ``%05d_upsampled.png``.  samples_per_ray / ms are those of the small plain render.
    Not with reproject_stride, supersample, sweep_scales, temporal or temporal_still.

    fovea (``R:N:T[,R:N:T...],N:T`` or what renderer.parse_fovea makes of it, or None): every frame is rendered with per-ray budgets around a
    gaze at the centre of the rendered frame (radii in its pixels).  Records and summary keep their shape: PSNR / FLIP / samples per ray are
    those of the foveated frames -- the quality-against-cost table of a foveation setting.

    fovea_density (``R:S[,R:S...],S`` or what renderer.parse_fovea_density makes of it, or None): foveated ray density beside the full
    frames.  After a pose's full render the same pose is rendered at the density of a gaze at the frame centre and reconstructed
    (NeuralRenderer.render_foveated), and that fp32 frame is scored too.  Records gain ``psnr_foveated`` / ``mse_foveated``,
    ``rendered_fraction`` (rays rendered, of w h), ``ms_foveated`` (the masked render's own time; the fill is not in it) and, with "flip",
    ``flip_foveated``; the summary ``mean_psnr_foveated``, ``mean_rendered_fraction``, ``mean_ms_foveated`` and ``mean_flip_foveated``;
    out_dir gets ``%05d_foveated.png``.  The plain keys are those of a run without the option.  Not with fovea (the masked render refuses
    budget maps), reproject_stride, supersample, sweep_scales, temporal, temporal_still or temporal_upsample.

    fovea_temporal (ALPHA in (0, 1] or None; needs fovea_density): beside the fill-only frame, the same pose once more through
    NeuralRenderer.render_foveated_temporal -- the lattice at the next phase of its 64-phase cycle, resolved against a history that knows
    which pixels were rendered (adanerf_temporal_resolve_sparse) -- the set in order as one sequence.  Records gain
    ``psnr_foveated_temporal`` / ``mse_foveated_temporal``, ``foveated_temporal_rejected_fraction`` and, with "flip",
    ``flip_foveated_temporal``; the summary their means; out_dir gets ``%05d_foveated_temporal.png``.
    fovea_temporal_still (K >= 1 or None): per pose instead, the frame after K such frames at rest from a cut; ALPHA is ``fovea_temporal``
    or, without it, 0.1; the summary carries ``fovea_temporal_still``.

    sweep_sample_caps (list of caps C or None): the set is rendered once per cap on the one context (NeuralRenderer.set_sample_cap: no
    frame shades more than C samples per ray on average; 0 = no cap), in the shape of sweep_samples.  The summary is ``{"frames": n,
    "sweep": [...]}`` with one ``{sample_cap, mean_psnr, mean_mse, mean_samples_per_ray, mean_cap_threshold, mean_ms[, mean_flip]}`` per cap;
    ``mean_cap_threshold`` is the mean over the trimmed frames of the largest threshold the cap chose (None if no frame was trimmed);
    records carry ``sample_cap`` and ``cap_threshold`` (None: not trimmed); out_dir gets ``cap<C>/``.  With metrics and fovea only; the cap
    is removed afterwards."""
    ip = int(interpolate_stride) if interpolate_stride is not None else 0
    if interpolate_stride is not None and (ip != interpolate_stride or ip < 1):
        raise ValueError("interpolate_stride must be an integer >= 1, got %s" % (interpolate_stride,))
    if ip and (reproject_stride is not None or supersample is not None or temporal is not None or temporal_still is not None or temporal_upsample is not None or
               fovea_density is not None or sweep_scales or sweep_thresholds or sweep_samples or sweep_sample_caps):
        raise ValueError("interpolate_stride makes frames from two keyframes at the dataset's resolution: not together with reproject_stride, supersample, "
                         "the temporal options, fovea_density or a sweep")
    if sweep_sample_caps and (sweep_thresholds or sweep_samples or sweep_scales or reproject_stride is not None or supersample is not None or
                              temporal is not None or temporal_still is not None or temporal_upsample is not None or fovea_density is not None):
        raise ValueError("sweep_sample_caps goes with metrics and fovea only")
    if sweep_sample_caps and not all(c == 0 or (math.isfinite(c) and c >= 1) for c in sweep_sample_caps):
        raise ValueError("sweep_sample_caps: every cap must be 0 or a finite value >= 1, got %s" % (list(sweep_sample_caps),))
    if isinstance(fovea, str):
        fovea = parse_fovea(fovea)
    if fovea_density is not None:
        fovea_density = parse_fovea_density(fovea_density) if isinstance(fovea_density, str) else parse_fovea_density(
            ",".join(":".join(str(int(v)) for v in ring) for ring in fovea_density))
    unknown = sorted(set(metrics) - {"psnr", "flip"})
    if unknown:
        raise ValueError("unknown metrics %s (known: psnr, flip)" % unknown)
    if sweep_scales and not all(s > 0 for s in sweep_scales):
        raise ValueError("sweep_scales must be positive, got %s" % (list(sweep_scales),))
    stride = int(reproject_stride) if reproject_stride is not None else 0
    if reproject_stride is not None and stride < 1:
        raise ValueError("reproject_stride must be >= 1, got %s" % (reproject_stride,))
    if rerender not in RERENDER_VALUES:
        raise ValueError("rerender must be None, 'holes' or 'unsourced', got %r" % (rerender,))
    if reproject_warp not in ("splat", "gather"):
        raise ValueError("reproject_warp must be 'splat' or 'gather', got %r" % (reproject_warp,))
    if (reproject_warp == "gather" or reproject_iterations is not None or reproject_tol is not None) and not stride:
        raise ValueError("reproject_warp / reproject_iterations / reproject_tol choose how warped frames are made: they need reproject_stride")
    gather_kw = dict(iterations=GATHER_ITERATIONS if reproject_iterations is None else int(reproject_iterations),
                     depth_tol=GATHER_DEPTH_TOL if reproject_tol is None else float(reproject_tol))
    if rerender and not stride and not ip:
        raise ValueError("rerender re-renders the holes of warped frames: it needs reproject_stride")
    if stride and sweep_scales:
        raise ValueError("reproject_stride warps at the dataset's resolution: not together with sweep_scales")
    ss = int(supersample) if supersample is not None else 0
    if supersample is not None and not 1 <= ss <= SUPERSAMPLE_MAX:
        raise ValueError("supersample must be in 1..%d, got %s" % (SUPERSAMPLE_MAX, supersample))
    contrast = None
    if supersample_contrast is not None:
        contrast = float(supersample_contrast)
        if not (np.isfinite(contrast) and 0.0 <= contrast <= 1.0):
            raise ValueError("supersample_contrast must lie in [0, 1], got %s" % (supersample_contrast,))
        if ss < 2:
            raise ValueError("supersample_contrast refines the edges of a supersampled frame: it needs supersample >= 2")
    if ss and stride:
        raise ValueError("supersample averages jittered frames, which have no single depth map to warp by: not together with reproject_stride")
    still = int(temporal_still) if temporal_still is not None else 0
    if temporal_still is not None and still < 1:
        raise ValueError("temporal_still must be >= 1, got %s" % (temporal_still,))
    ta = (0.1 if temporal is None else float(temporal)) if (temporal is not None or still) else 0.0
    if temporal is not None and not 0.0 < ta <= 1.0:
        raise ValueError("temporal must lie in (0, 1], got %s" % (temporal,))
    if ta and (stride or ss or sweep_scales):
        raise ValueError("temporal / temporal_still resolve one jittered render per frame at the dataset's resolution: not together with "
                         "reproject_stride, supersample or sweep_scales")
    tu = int(temporal_upsample) if temporal_upsample is not None else 0
    if temporal_upsample is not None and (tu != temporal_upsample or not 1 <= tu <= 4):
        raise ValueError("temporal_upsample must be 1, 2, 3 or 4, got %s" % (temporal_upsample,))
    if temporal_upsample_frames is not None and (not tu or int(temporal_upsample_frames) != temporal_upsample_frames or temporal_upsample_frames < 1):
        raise ValueError("temporal_upsample_frames must be an integer >= 1 and goes with temporal_upsample, got %s" % (temporal_upsample_frames,))
    tu_frames = int(temporal_upsample_frames) if temporal_upsample_frames is not None else tu * tu
    if tu and (stride or ss or sweep_scales or ta):
        raise ValueError("temporal_upsample renders at the dataset's size / S and resolves at the dataset's size: not together with "
                         "reproject_stride, supersample, sweep_scales, temporal or temporal_still")
    if fovea_density and (fovea or stride or ss or sweep_scales or ta or tu):
        raise ValueError("fovea_density renders a lattice of whole frames at the dataset's resolution without budget maps: not together with "
                         "fovea, reproject_stride, supersample, sweep_scales, temporal, temporal_still or temporal_upsample")
    ft_still = int(fovea_temporal_still) if fovea_temporal_still is not None else 0
    if fovea_temporal_still is not None and (ft_still != fovea_temporal_still or ft_still < 1):
        raise ValueError("fovea_temporal_still must be an integer >= 1, got %s" % (fovea_temporal_still,))
    ft = (0.1 if fovea_temporal is None else float(fovea_temporal)) if (fovea_temporal is not None or ft_still) else 0.0
    if fovea_temporal is not None and not 0.0 < ft <= 1.0:
        raise ValueError("fovea_temporal must lie in (0, 1], got %s" % (fovea_temporal,))
    if ft and not fovea_density:
        raise ValueError("fovea_temporal / fovea_temporal_still resolve the frames of a moving lattice: they need fovea_density")
    if present_filter not in PRESENT_FILTERS:
        raise ValueError("present_filter must be None, 'nearest', 'linear' or 'area', got %r" % (present_filter,))
    want_flip = "flip" in metrics
    meta, frames = load_dataset(dataset_dir, set_name)
    if max_frames > 0:
        frames = frames[:max_frames]
    w, h = meta["w"], meta["h"]
    if tu and (w % tu or h % tu):
        raise ValueError("temporal_upsample %d does not divide the dataset's %d x %d" % (tu, w, h))
    results: List[dict] = []
    with NeuralRenderer(Settings(model_dir, w // tu if tu else w, h // tu if tu else h, batch_size=batch_size), precision=precision) as r:
        if abs(r.info.fov - meta["fov"]) > 1e-4 and not quiet:
            print("warning: dataset camera_angle_x %.6f differs from the model's fov %.6f (the model's is used)" %
                  (meta["fov"], r.info.fov), file=sys.stderr)
        vid = Y4mWriter(video, w, h, fps) if video else None
        d_ref = r.empty((w * h, 3), np.float32) if want_flip else None
        d_map = r.empty((w * h,), np.float32) if want_flip and out_dir else None
        d_pres = r.empty((w * h, 3), np.float32) if want_flip and (sweep_scales or stride or ta or tu or ft or ip) else None      # (the foveated frame is scored in place)
        if stride:
            r.enable_reprojection()
        if ip:
            r.enable_interpolation()
        if ta:
            r.enable_temporal(alpha=ta, grid=2)
        if tu:
            r.enable_temporal_upsample(scale=tu)

        def render_set(out_dir, extra, scale=None):
            """one pass over the set at the selection (and, with a scale, the frame size) in force -> its records"""
            rw, rh = (w, h) if scale is None and not tu else (r.info.width, r.info.height)
            presented = scale is not None or bool(tu)
            recs: List[dict] = []
            if out_dir:
                os.makedirs(out_dir, exist_ok=True)
            if fovea:      # again for every setting: a frame size that changes the ray count drops the maps
                r.foveate((0.5 * rw, 0.5 * rh), fovea)
            if ta:
                r.reset_temporal()      # a pass over the set is one sequence
            if fovea_density:      # again for every setting: the mask belongs to the frame size
                r.foveate_density((0.5 * rw, 0.5 * rh), fovea_density)
            if ft:      # a pass over the set is one sequence, from a cut
                r.enable_foveated_temporal(alpha=ft)
            keys = [i for i in range(len(frames)) if i % ip == 0 or i == len(frames) - 1] if ip else []
            order = list(range(len(frames)))
            if ip:      # every keyframe ahead of the poses it closes: the frame after an in-between pose is rendered before that pose is made
                order = sorted(order, key=lambda i: (min(k for k in keys if k >= i) if i else 0, i not in keys, i))
            for i in order:
                fr = frames[i]
                ref = None
                warped = bool(stride) and i % stride != 0
                interpolated = bool(ip) and i not in keys
                if interpolated:      # between the keyframe before this pose and the keyframe after it
                    rgb, rgba, _, source, holes = r.interpolate(fr["pose"], fr["rot"])
                    rec = dict(extra, frame=i, image=fr["image"], interpolated=True, hole_fraction=holes / float(w * h),
                               blended_fraction=int(np.count_nonzero(source == 3)) / float(w * h))
                    if rerender:
                        rr_rgb, rr_rgba, _, _, _, rerendered = r.interpolate_rerender(fr["pose"], fr["rot"], rerender)
                        rec.update(rerendered_fraction=rerendered / float(w * h))
                        if out_dir:
                            write_png(os.path.join(out_dir, "%05d_rerendered.png" % i), rr_rgba[:, :3].reshape(h, w, 3))
                elif ip:
                    r.set_camera(fr["pose"], fr["rot"])
                    rgb, rgba, st = r.render_keyframe()
                    rec = dict(extra, frame=i, image=fr["image"], samples_per_ray=st.total_samples / float(rw * rh), ms=st.ms_total, interpolated=False)
                elif warped:      # the last rendered frame at this pose: what a host that renders every K-th frame shows here
                    if reproject_warp == "gather":
                        _, rgba, _, holes = r.reproject_gather(fr["pose"], fr["rot"], **gather_kw)
                    else:
                        rgba, _, holes = r.reproject(fr["pose"], fr["rot"])
                    rgb = rgba[:, :3].astype(np.float32) / 255.0
                    rec = dict(extra, frame=i, image=fr["image"], warped=True, warp=reproject_warp, hole_fraction=holes / float(w * h))
                    if rerender:      # the same warp with its holes rendered at this pose
                        if reproject_warp == "gather":
                            rr_rgba, _, _, rerendered = r.reproject_gather_rerender(fr["pose"], fr["rot"], rerender, **gather_kw)
                        else:
                            rr_rgba, _, _, rerendered = r.reproject_rerender(fr["pose"], fr["rot"], rerender)
                        rr_rgb = rr_rgba[:, :3].astype(np.float32) / 255.0
                        rec.update(rerendered_fraction=rerendered / float(w * h))
                        if out_dir:
                            os.makedirs(out_dir, exist_ok=True)
                            write_png(os.path.join(out_dir, "%05d_rerendered.png" % i), rr_rgba[:, :3].reshape(h, w, 3))
                else:
                    r.set_camera(fr["pose"], fr["rot"])
                    if contrast is not None:
                        rgb, rgba, _, refined, st = r.render_supersampled_adaptive(ss, contrast)
                    else:
                        rgb, rgba, st = r.render_supersampled(ss) if ss else r.render_numpy()
                    if presented:      # the frame as a w x h window shows it, filtered on the device
                        rgba = r.present(w, h, filter="linear" if tu else present_filter).reshape(-1, 4)
                        rgb = rgba[:, :3].astype(np.float32) / 255.0
                    rec = dict(extra, frame=i, image=fr["image"], samples_per_ray=st.total_samples / float(rw * rh), ms=st.ms_total)
                    if "sample_cap" in extra:      # the largest threshold the cap chose over the frame's batches
                        t_cap = float(r.sample_cap_report().threshold_max)
                        rec.update(cap_threshold=t_cap if math.isfinite(t_cap) or t_cap > 0 else None)
                    if stride:
                        rec.update(warped=False)
                    if ss:
                        rec.update(supersample=ss)
                    if contrast is not None:
                        rec.update(refined_fraction=refined / float(rw * rh))
                if os.path.exists(fr["image"]):
                    gt = read_png(fr["image"])
                    if gt.shape[0] != h or gt.shape[1] != w:
                        raise ValueError("%s: expected %dx%d, got %dx%d" % (fr["image"], w, h, gt.shape[1], gt.shape[0]))
                    ref = gt[:, :, :3].astype(np.float32).reshape(-1, 3) / 255.0        # datasets.py:286-287
                    mse = float(np.mean((rgb.astype(np.float64) - ref) ** 2))
                    rec.update(mse=mse, psnr=psnr_from_mse(mse))
                    if (warped or interpolated) and rerender:
                        rr_mse = float(np.mean((rr_rgb.astype(np.float64) - ref) ** 2))
                        rec.update(mse_rerendered=rr_mse, psnr_rerendered=psnr_from_mse(rr_mse))
                    if want_flip:       # the rendered frame is still on the device (render_numpy); argument order of src/evaluate.py:144
                        d_test = r._o_rgb if not presented and not warped and not ip else d_pres.upload(rgb)
                        rec.update(flip=r.flip_device(d_test, d_ref.upload(ref), w, h, error_map=d_map))
                        if d_map is not None:
                            fm = np.nan_to_num(d_map.numpy().reshape(h, w), nan=1.0)      # the map lies in [0, 1]
                            write_png(os.path.join(out_dir, "%05d_flip.png" % i), np.clip(np.rint(fm * 255.0), 0, 255).astype(np.uint8))
                if ta:      # the same pose once more, jittered, resolved against the history (or K times from an empty one)
                    if still:
                        r.reset_temporal()
                    for _ in range(still or 1):
                        t_rgb, t_rgba, _, t_rejected, _ = r.render_temporal()
                    rec.update(rejected_fraction=t_rejected / float(w * h))
                    if ref is not None:
                        t_mse = float(np.mean((t_rgb.astype(np.float64) - ref) ** 2))
                        rec.update(mse_temporal=t_mse, psnr_temporal=psnr_from_mse(t_mse))
                        if want_flip:
                            rec.update(flip_temporal=r.flip_device(d_pres.upload(t_rgb), d_ref, w, h))
                    if out_dir:
                        write_png(os.path.join(out_dir, "%05d_temporal.png" % i), t_rgba[:, :3].reshape(h, w, 3))
                if tu:      # the same pose, at rest from an empty history: K jittered small renders resolved at the dataset's size
                    r.reset_upsample()
                    for _ in range(tu_frames):
                        u_rgb, u_rgba, _, u_rejected, _ = r.render_upsampled()
                    rec.update(temporal_upsample=tu, rejected_fraction=u_rejected / float(w * h))
                    if ref is not None:
                        u_mse = float(np.mean((u_rgb.astype(np.float64) - ref) ** 2))
                        rec.update(mse_upsampled=u_mse, psnr_upsampled=psnr_from_mse(u_mse))
                        if want_flip:
                            rec.update(flip_upsampled=r.flip_device(d_pres.upload(u_rgb), d_ref, w, h))
                    if out_dir:
                        write_png(os.path.join(out_dir, "%05d_upsampled.png" % i), u_rgba[:, :3].reshape(h, w, 3))
                if fovea_density:      # the same pose at the gaze's ray density, reconstructed; after the full frame's scores: it reuses its images
                    f_rgb, f_rgba, f_rendered, f_st = r.render_foveated()
                    rec.update(rendered_fraction=f_rendered / float(w * h), ms_foveated=f_st.ms_total)
                    if ref is not None:
                        f_mse = float(np.mean((f_rgb.astype(np.float64) - ref) ** 2))
                        rec.update(mse_foveated=f_mse, psnr_foveated=psnr_from_mse(f_mse))
                        if want_flip:
                            rec.update(flip_foveated=r.flip_device(r._o_rgb, d_ref, w, h))
                    if out_dir:
                        write_png(os.path.join(out_dir, "%05d_foveated.png" % i), f_rgba[:, :3].reshape(h, w, 3))
                if ft:      # the same pose once more on the lattice of the next phase, resolved against the history (or K times from a cut)
                    if ft_still:
                        r.reset_foveated_temporal()
                    for _ in range(ft_still or 1):
                        s_rgb, s_rgba, _, s_rejected, _, _ = r.render_foveated_temporal()
                    rec.update(foveated_temporal_rejected_fraction=s_rejected / float(w * h))
                    if ref is not None:
                        s_mse = float(np.mean((s_rgb.astype(np.float64) - ref) ** 2))
                        rec.update(mse_foveated_temporal=s_mse, psnr_foveated_temporal=psnr_from_mse(s_mse))
                        if want_flip:
                            rec.update(flip_foveated_temporal=r.flip_device(d_pres.upload(s_rgb), d_ref, w, h))
                    if out_dir:
                        write_png(os.path.join(out_dir, "%05d_foveated_temporal.png" % i), s_rgba[:, :3].reshape(h, w, 3))
                if out_dir:
                    write_png(os.path.join(out_dir, "%05d.png" % i), rgba[:, :3].reshape(h, w, 3))
                if vid:
                    vid.add(rgba[:, :3].reshape(h, w, 3))
                recs.append(rec)
                if not quiet:
                    print("frame %d: %s" % (i, ", ".join("%s=%s" % (k, ("%.4f" % v) if isinstance(v, float) else v)
                                                          for k, v in rec.items() if k not in ("frame", "image"))))
            return sorted(recs, key=lambda x: x["frame"]) if ip else recs

        sweep = []
        if sweep_thresholds or sweep_samples or sweep_scales:
            for n, t, sc in itertools.product(sweep_samples or [None], sweep_thresholds or [None], sweep_scales or [None]):
                info = r.set_selection(n, t)
                key = dict(num_samples=int(info.num_samples), threshold=float(info.threshold) if t is None else float(t))
                if sc is not None:
                    r.set_frame_size(*scaled_size(w, h, sc))
                    key["scale"] = float(sc)
                recs = render_set(os.path.join(out_dir, sweep_dir_name(**key)) if out_dir else None, key, sc)
                sweep.append(dict(key, **{k: v for k, v in summarise(recs, want_flip).items() if k != "frames"}, **(dict(supersample=ss) if ss else {})))
                results.extend(recs)
        elif sweep_sample_caps:
            try:
                for cap in sweep_sample_caps:
                    r.set_sample_cap(cap)
                    key = dict(sample_cap=float(cap))
                    recs = render_set(os.path.join(out_dir, "cap%g" % cap) if out_dir else None, key)
                    trimmed = [x["cap_threshold"] for x in recs if x.get("cap_threshold") is not None]
                    sweep.append(dict(key, **{k: v for k, v in summarise(recs, want_flip).items() if k != "frames"},
                                      mean_cap_threshold=float(np.mean(trimmed)) if trimmed else None))
                    results.extend(recs)
            finally:
                r.set_sample_cap(0)
        else:
            results = render_set(out_dir, {})
        if vid:
            vid.close()
    if sweep:
        return dict(frames=len(frames), sweep=sweep, **(dict(supersample=ss) if ss else {}), **(dict(temporal_still=still) if still else {})), results
    return dict(summarise(results, want_flip), **(dict(supersample=ss) if ss else {}), **(dict(temporal_still=still) if still else {}),
                **(dict(temporal_upsample=tu, temporal_upsample_frames=tu_frames) if tu else {}),
                **(dict(fovea_temporal_still=ft_still) if ft_still else {})), results


def summarise(results: List[dict], want_flip: bool) -> dict:
    with_gt = [x for x in results if "psnr" in x]
    rendered = [x for x in results if not x.get("warped") and not x.get("interpolated")]
    summary = dict(frames=len(results), mean_samples_per_ray=float(np.mean([x["samples_per_ray"] for x in rendered])) if rendered else 0.0,
                   mean_ms=float(np.mean([x["ms"] for x in rendered])) if rendered else 0.0)
    if with_gt:
        summary.update(mean_psnr=float(np.mean([x["psnr"] for x in with_gt])), mean_mse=float(np.mean([x["mse"] for x in with_gt])))
        if want_flip:
            summary.update(mean_flip=float(np.mean([x["flip"] for x in with_gt])))
    if any("warped" in x for x in results):      # reproject_stride: the two kinds of frame apart (None: no such frame with a ground truth)
        for kind, flag in (("rendered", False), ("warped", True)):
            part = [x for x in with_gt if bool(x.get("warped")) == flag]
            summary["mean_psnr_" + kind] = float(np.mean([x["psnr"] for x in part])) if part else None
            if want_flip:
                summary["mean_flip_" + kind] = float(np.mean([x["flip"] for x in part])) if part else None
        holes = [x["hole_fraction"] for x in results if x.get("warped")]
        summary["mean_hole_fraction"] = float(np.mean(holes)) if holes else 0.0
        if any("rerendered_fraction" in x for x in results):      # rerender: the warped frames once more, their holes rendered
            part = [x["psnr_rerendered"] for x in results if "psnr_rerendered" in x]
            summary["mean_psnr_warped_rerendered"] = float(np.mean(part)) if part else None
            summary["mean_rerendered_fraction"] = float(np.mean([x["rerendered_fraction"] for x in results if "rerendered_fraction" in x]))
    if any("interpolated" in x for x in results):      # interpolate_stride: the keyframes and the frames made between them apart
        for kind, flag in (("rendered", False), ("interpolated", True)):
            part = [x for x in with_gt if bool(x.get("interpolated")) == flag]
            summary["mean_psnr_" + kind] = float(np.mean([x["psnr"] for x in part])) if part else None
            if want_flip:
                summary["mean_flip_" + kind] = float(np.mean([x["flip"] for x in part])) if part else None
        made = [x for x in results if x.get("interpolated")]
        summary["mean_hole_fraction"] = float(np.mean([x["hole_fraction"] for x in made])) if made else 0.0
        summary["mean_blended_fraction"] = float(np.mean([x["blended_fraction"] for x in made])) if made else 0.0
        if any("rerendered_fraction" in x for x in results):
            part = [x["psnr_rerendered"] for x in results if "psnr_rerendered" in x]
            summary["mean_psnr_interpolated_rerendered"] = float(np.mean(part)) if part else None
            summary["mean_rerendered_fraction"] = float(np.mean([x["rerendered_fraction"] for x in results if "rerendered_fraction" in x]))
    if any("temporal_upsample" in x for x in results):      # temporal_upsample: the upsampled frames beside the enlarged small ones
        part = [x for x in results if "psnr_upsampled" in x]
        summary["mean_psnr_upsampled"] = float(np.mean([x["psnr_upsampled"] for x in part])) if part else None
        if want_flip:
            summary["mean_flip_upsampled"] = float(np.mean([x["flip_upsampled"] for x in part])) if part else None
        summary["mean_rejected_fraction"] = float(np.mean([x["rejected_fraction"] for x in results if "rejected_fraction" in x]))
    elif any("rejected_fraction" in x for x in results):      # temporal / temporal_still: the resolved frames beside the plain ones
        part = [x for x in results if "psnr_temporal" in x]
        summary["mean_psnr_temporal"] = float(np.mean([x["psnr_temporal"] for x in part])) if part else None
        if want_flip:
            summary["mean_flip_temporal"] = float(np.mean([x["flip_temporal"] for x in part])) if part else None
        summary["mean_rejected_fraction"] = float(np.mean([x["rejected_fraction"] for x in results if "rejected_fraction" in x]))
    if any("rendered_fraction" in x for x in results):      # fovea_density: the reconstructed frames beside the full ones
        part = [x for x in results if "psnr_foveated" in x]
        summary["mean_psnr_foveated"] = float(np.mean([x["psnr_foveated"] for x in part])) if part else None
        if want_flip:
            summary["mean_flip_foveated"] = float(np.mean([x["flip_foveated"] for x in part])) if part else None
        summary["mean_rendered_fraction"] = float(np.mean([x["rendered_fraction"] for x in results if "rendered_fraction" in x]))
        summary["mean_ms_foveated"] = float(np.mean([x["ms_foveated"] for x in results if "ms_foveated" in x]))
    if any("foveated_temporal_rejected_fraction" in x for x in results):      # fovea_temporal: the resolved frames beside the fill-only ones
        part = [x for x in results if "psnr_foveated_temporal" in x]
        summary["mean_psnr_foveated_temporal"] = float(np.mean([x["psnr_foveated_temporal"] for x in part])) if part else None
        if want_flip:
            summary["mean_flip_foveated_temporal"] = float(np.mean([x["flip_foveated_temporal"] for x in part])) if part else None
        summary["mean_foveated_temporal_rejected_fraction"] = float(np.mean([x["foveated_temporal_rejected_fraction"] for x in results
                                                                             if "foveated_temporal_rejected_fraction" in x]))
    if any("refined_fraction" in x for x in results):      # supersample_contrast: the share of the pixels that got the S x S renders
        summary["mean_refined_fraction"] = float(np.mean([x["refined_fraction"] for x in results if "refined_fraction" in x]))
    return summary


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("model_dir")
    ap.add_argument("dataset_dir")
    ap.add_argument("--set", default="test")
    ap.add_argument("--out", default=None, help="write the rendered frames as PNG here")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--batch-size", type=int, default=-1)
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--video", default=None, help="also write the rendered frames as an uncompressed .y4m video")
    ap.add_argument("--fps", type=int, default=30)
    ap.add_argument("--metrics", nargs="+", default=["psnr"], choices=["psnr", "flip"],
                    help="flip: also the mean FLIP error per frame (and, with --out, its map as %%05d_flip.png)")
    ap.add_argument("--sweep-thresholds", nargs="+", type=float, default=None, metavar="T",
                    help="render the set once per threshold (x --sweep-samples) on one context; summary gains `sweep`, --out gets n<N>_t<T>/")
    ap.add_argument("--sweep-samples", nargs="+", type=int, default=None, metavar="N",
                    help="render the set once per sample budget N (x --sweep-thresholds)")
    ap.add_argument("--sweep-sample-caps", nargs="+", type=float, default=None, metavar="C",
                    help="render the set once per sample cap C (mean samples per ray no frame may exceed; 0 = none) on one context; summary "
                         "gains `sweep` with mean_cap_threshold, --out gets cap<C>/")
    ap.add_argument("--sweep-scales", nargs="+", type=float, default=None, metavar="S",
                    help="render the set once per scale S of the dataset's resolution (x the other sweeps) on the same context, present it "
                         "to the full size on the GPU and score that 8-bit image; entries gain `scale`, --out directories _s<S>")
    ap.add_argument("--reproject-stride", type=int, default=None, metavar="K",
                    help="render the poses with i %% K == 0 and warp the others from the nearest rendered pose before them (adanerf_reproject); "
                         "the summary gains mean_psnr_rendered / mean_psnr_warped / mean_hole_fraction (and mean_flip_* with --metrics flip)")
    ap.add_argument("--reproject-warp", default=None, choices=["splat", "gather"],
                    help="with --reproject-stride: how the warped frames are made -- splat (default, adanerf_reproject) or gather "
                         "(adanerf_reproject_gather: every pixel iterates along its ray to the source surface); warped records carry `warp`")
    ap.add_argument("--reproject-iterations", type=int, default=None, metavar="N", help="with --reproject-warp gather: steps per pixel, 1..8 (default %d)" % GATHER_ITERATIONS)
    ap.add_argument("--reproject-tol", type=float, default=None, metavar="T",
                    help="with --reproject-warp gather: relative depth tolerance of the consistency test (default %g)" % GATHER_DEPTH_TOL)
    ap.add_argument("--interpolate-stride", type=int, default=None, metavar="K",
                    help="render the poses with i %% K == 0 and the last one as keyframes and make the others from the keyframe before AND the keyframe "
                         "after them (adanerf_reproject_pair); the summary gains mean_psnr_rendered / mean_psnr_interpolated / mean_hole_fraction / "
                         "mean_blended_fraction (and mean_flip_* with --metrics flip); --rerender applies to those frames")
    ap.add_argument("--rerender", default=None, choices=["holes", "unsourced"],
                    help="with --reproject-stride: score every warped frame once more with its holes (unsourced: the filled pixels too) rendered at "
                         "its own pose (adanerf_render_masked); the summary gains mean_psnr_warped_rerendered / mean_rerendered_fraction")
    ap.add_argument("--supersample", type=int, default=None, choices=range(1, SUPERSAMPLE_MAX + 1), metavar="S",
                    help="every image is the mean of S x S renders (S in 1..8) at the offsets of the regular sub-pixel grid, accumulated on the GPU "
                         "and scored from the fp32 mean; records and summary gain `supersample`; not together with --reproject-stride")
    ap.add_argument("--temporal", type=float, default=None, metavar="ALPHA",
                    help="temporal anti-aliasing beside the plain frames: the set in order as one sequence, every pose rendered once more at the "
                         "next sub-pixel offset and resolved against the history (adanerf_temporal_resolve, new-frame weight ALPHA in (0, 1]); the "
                         "summary gains mean_psnr_temporal / mean_rejected_fraction (and mean_flip_temporal with --metrics flip)")
    ap.add_argument("--temporal-still", type=int, default=None, metavar="K",
                    help="per pose, score the frame after K resolves at rest from an empty history instead (ALPHA of --temporal, default 0.1)")
    ap.add_argument("--temporal-upsample", type=int, default=None, choices=range(1, 5), metavar="S",
                    help="temporal upsampling beside the plain frames: render at the dataset's size / S (which must divide), per pose resolve K "
                         "jittered frames at rest at the dataset's size (adanerf_temporal_upsample) and score that frame; the plain frame is the "
                         "un-jittered small render enlarged by the linear present filter; the summary gains mean_psnr_upsampled / "
                         "mean_rejected_fraction (and mean_flip_upsampled with --metrics flip)")
    ap.add_argument("--temporal-upsample-frames", type=int, default=None, metavar="K", help="frames resolved per pose (default S x S)")
    ap.add_argument("--present-filter", default=None, choices=["nearest", "linear", "area"],
                    help="filter of the --sweep-scales presentation (default: the viewer's rule, linear when enlarging, else nearest); area is "
                         "the exact area filter and the only sensible choice for scales above 1, where nearest throws the extra rays away")
    ap.add_argument("--fovea", type=parse_fovea, default=None, metavar="R:N:T[,R:N:T...],N:T",
                    help="per-ray sample budgets around a gaze at the image centre: rings (radius px : N : threshold), then the entry outside "
                         "them; PSNR / FLIP / samples per ray are then those of the foveated frames")
    ap.add_argument("--fovea-density", default=None, metavar="R:S[,R:S...],S",
                    help="foveated ray density beside the full frames, gaze at the frame centre: rings (radius px : stride 1|2|4|8), then the "
                         "stride outside them; every pose is rendered once more on that lattice and reconstructed (adanerf_foveate_density / "
                         "adanerf_render_masked / adanerf_fill_density); the summary gains mean_psnr_foveated / mean_rendered_fraction / "
                         "mean_ms_foveated (and mean_flip_foveated with --metrics flip)")
    ap.add_argument("--fovea-temporal", type=float, default=None, metavar="ALPHA",
                    help="with --fovea-density: every pose once more on the lattice of the next phase of its 64-phase cycle, resolved against a "
                         "history that knows which pixels were rendered (adanerf_temporal_resolve_sparse, rendered-pixel weight ALPHA in (0, 1]); "
                         "the summary gains mean_psnr_foveated_temporal / mean_foveated_temporal_rejected_fraction beside mean_psnr_foveated")
    ap.add_argument("--fovea-temporal-still", type=int, default=None, metavar="K",
                    help="per pose, score the frame after K such frames at rest from a cut instead (ALPHA of --fovea-temporal, default 0.1)")
    ap.add_argument("--supersample-contrast", type=float, default=None, metavar="T",
                    help="with --supersample S >= 2: adaptive supersampling -- one render at the pixel centres, the S x S renders only for the "
                         "pixels a neighbour of which differs by more than T (0..1) in some channel (adanerf_contrast_mask / "
                         "adanerf_render_masked); the summary gains mean_refined_fraction")
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if (a.reproject_warp is not None or a.reproject_iterations is not None or a.reproject_tol is not None) and a.reproject_stride is None:
        ap.error("--reproject-warp / --reproject-iterations / --reproject-tol need --reproject-stride")
    if a.rerender is not None and a.reproject_stride is None and a.interpolate_stride is None:
        ap.error("--rerender needs --reproject-stride")
    if a.interpolate_stride is not None and (a.reproject_stride is not None or a.supersample is not None or a.temporal is not None or a.temporal_still is not None or
                                             a.temporal_upsample is not None or a.fovea_density is not None or a.sweep_scales or a.sweep_thresholds or
                                             a.sweep_samples or a.sweep_sample_caps):
        ap.error("--interpolate-stride cannot be combined with --reproject-stride, --supersample, the --temporal options, --fovea-density or a sweep")
    if a.supersample is not None and a.reproject_stride is not None:
        ap.error("--supersample cannot be combined with --reproject-stride")
    if (a.temporal is not None or a.temporal_still is not None) and (a.supersample is not None or a.reproject_stride is not None or a.sweep_scales):
        ap.error("--temporal / --temporal-still cannot be combined with --supersample, --reproject-stride or --sweep-scales")
    if a.temporal_upsample is not None and (a.temporal is not None or a.temporal_still is not None or a.supersample is not None or
                                            a.reproject_stride is not None or a.sweep_scales):
        ap.error("--temporal-upsample cannot be combined with --temporal, --temporal-still, --supersample, --reproject-stride or --sweep-scales")
    if a.fovea_density is not None:
        try:
            parse_fovea_density(a.fovea_density)
        except ValueError as e:
            ap.error(str(e))
        if (a.fovea is not None or a.reproject_stride is not None or a.supersample is not None or a.sweep_scales or a.temporal is not None or
                a.temporal_still is not None or a.temporal_upsample is not None):
            ap.error("--fovea-density cannot be combined with --fovea, --reproject-stride, --supersample, --sweep-scales or the --temporal options")
    if (a.fovea_temporal is not None or a.fovea_temporal_still is not None) and a.fovea_density is None:
        ap.error("--fovea-temporal / --fovea-temporal-still need --fovea-density")
    if a.fovea_temporal is not None and not 0.0 < a.fovea_temporal <= 1.0:
        ap.error("--fovea-temporal ALPHA: ALPHA must lie in (0, 1]")
    if a.fovea_temporal_still is not None and a.fovea_temporal_still < 1:
        ap.error("--fovea-temporal-still K: K must be >= 1")
    if a.supersample_contrast is not None:
        if a.supersample is None or a.supersample < 2:
            ap.error("--supersample-contrast requires --supersample S with S >= 2")
        if not (np.isfinite(a.supersample_contrast) and 0.0 <= a.supersample_contrast <= 1.0):
            ap.error("--supersample-contrast T: T must lie in [0, 1]")
    if a.temporal_upsample_frames is not None and a.temporal_upsample is None:
        ap.error("--temporal-upsample-frames goes with --temporal-upsample")
    summary, _ = evaluate(a.model_dir, a.dataset_dir, a.set, a.out, a.precision, a.batch_size, a.max_frames, video=a.video, fps=a.fps,
                          metrics=tuple(a.metrics), sweep_thresholds=a.sweep_thresholds, sweep_samples=a.sweep_samples, sweep_scales=a.sweep_scales,
                          fovea=a.fovea, reproject_stride=a.reproject_stride, reproject_warp=a.reproject_warp or "splat", reproject_iterations=a.reproject_iterations,
                          reproject_tol=a.reproject_tol, rerender=a.rerender, supersample=a.supersample, present_filter=a.present_filter,
                          temporal=a.temporal, temporal_still=a.temporal_still, temporal_upsample=a.temporal_upsample,
                          temporal_upsample_frames=a.temporal_upsample_frames, fovea_density=a.fovea_density,
                          supersample_contrast=a.supersample_contrast, fovea_temporal=a.fovea_temporal, fovea_temporal_still=a.fovea_temporal_still,
                          sweep_sample_caps=a.sweep_sample_caps, interpolate_stride=a.interpolate_stride)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
