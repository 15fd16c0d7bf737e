"""ctypes host mirror of the reference viewer's object model over the C ABI (include/adanerf_hip.h).

Names follow adanerf_real_time_viewer: ``Settings`` (include/settings.h:12-34, CLI semantics of
src/settings.cpp:15-47) and ``NeuralRenderer`` with ``init()`` / ``render()``
(include/neuralrenderer.h:53-55).  Stage-level methods mirror the reference launchers
(include/cuda/adanerf_cuda_kernels.cuh:20-74) and exist for the parity tests.

The product path is the HIP library.  Nothing here falls back to a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .build import library_path

PREC_BF16, PREC_FP16, PREC_FP32 = 0, 1, 2
_PREC = {"bf16": PREC_BF16, "fp16": PREC_FP16, "f16": PREC_FP16, "fp32": PREC_FP32, "f32": PREC_FP32}

BUF_RAYS, BUF_ORACLE, BUF_RAY_OFFSETS, BUF_RAY_COUNTS, BUF_SAMPLE_KEY, BUF_SAMPLE_W, BUF_RAW, BUF_TOTAL, BUF_SAMPLE_Z, BUF_RAW_COARSE = range(10)
BUF_RAY_LIST, BUF_RAY_LIST_COUNT = 10, 11                      # adanerf_render_masked: the ascending ray ids of the last call, their number
SAMPLER_ADAPTIVE, SAMPLER_PDF, SAMPLER_COARSE_FINE = 0, 1, 2
FLAG_KEEP_ORACLE, FLAG_WAVE_SELECT, FLAG_NO_GUARD_CACHE, FLAG_GUARD_AUDIT_FILL = 1, 2, 4, 8
PRESENT_FLIP_Y, PRESENT_NEAREST, PRESENT_LINEAR, PRESENT_AREA = 1, 2, 4, 8      # adanerf_present flags
PRESENT_FILTERS = {None: 0, "nearest": PRESENT_NEAREST, "linear": PRESENT_LINEAR, "area": PRESENT_AREA}
SUPERSAMPLE_MAX = 8                                            # adanerf_host_subpixel_grid: s in 1..8
REPROJECT_FILL = 1                                             # adanerf_reproject flag
GATHER_GUESS = 1                                               # adanerf_reproject_gather flag
GATHER_ITERATIONS, GATHER_DEPTH_TOL = 4, 0.05                  # the hosts' defaults (profiles/reproject_gather_measured.md)
RERENDER_VALUES = {None: 0, "holes": 1, "unsourced": 5}        # adanerf_render_masked `values` over adanerf_reproject's mask bytes (0 hole, 2 filled)
TEMPORAL_CLAMP = 1                                          # adanerf_temporal_resolve flag
ABI_VERSION = 4
GUARD_FROM = {0: "none", 1: "options", 2: "record", 3: "calibration", 4: "monitor"}
SAMPLING_MODES = {"split": 0, "fp16x3": 0, "fp32": 1, "fp16": 2, "guarded": 3}
# The default rule: the sampling mode that is exact by construction (split) unless the guarded mode is at least this much faster ON THE
# WORKLOAD AT HAND -- choose_sampling() measures it; `sampling="auto"` / `adanerf --sampling auto` apply it.
DEFAULT_RULE_MARGIN = 0.08


class AdaNeRFError(RuntimeError):
    pass


class _Options(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("batch_rays", C.c_int32), ("device_id", C.c_int32),
                ("precision", C.c_int32), ("num_samples", C.c_int32), ("threshold", C.c_float),
                ("shard_rank", C.c_int32), ("shard_world", C.c_int32), ("strip_rows", C.c_int32),
                ("sampling_mode", C.c_int32), ("flags", C.c_int32), ("guard_eps", C.c_float), ("guard_eps_pair", C.c_float),
                ("guard_audit_period", C.c_int32), ("reserved", C.c_int32 * 1)]


class Info(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("rays_local", C.c_int32),
                ("rays_local_max", C.c_int32), ("batch_rays", C.c_int32), ("n_in0", C.c_int32), ("n_in1", C.c_int32),
                ("num_samples", C.c_int32), ("threshold", C.c_float), ("dense", C.c_int32), ("use_ndc", C.c_int32),
                ("precision", C.c_int32), ("compute_units", C.c_int32), ("fov", C.c_float), ("focal", C.c_float),
                ("view_cell_center", C.c_float * 3), ("view_cell_radius", C.c_float), ("depth_range", C.c_float * 2),
                ("max_depth", C.c_float), ("sampler_mode", C.c_int32), ("view_cell_size", C.c_float * 3), ("num_samples_coarse", C.c_int32), ("guard_eps", C.c_float),
                ("guard_eps_pair", C.c_float), ("guard_audit_period", C.c_int32), ("guard_calib_source", C.c_int32), ("guard_calib_poses", C.c_int32),
                ("reserved", C.c_int32 * 8)]


class Stats(C.Structure):
    _fields_ = [("total_samples", C.c_int64), ("rays", C.c_int32), ("batches", C.c_int32), ("ms_total", C.c_float),
                ("ms_sample_mlp", C.c_float), ("ms_compact", C.c_float), ("ms_shade_mlp", C.c_float),
                ("ms_composite", C.c_float), ("shade_launches", C.c_int32), ("sample_launches", C.c_int32),
                ("sampling_overflow", C.c_int32), ("rays_refined", C.c_int32), ("guard_max_seen", C.c_float),
                ("guard_violations", C.c_int32), ("guard_widened", C.c_int32), ("guard_pair_seen", C.c_float), ("guard_audited", C.c_int32),
                ("guard_audit_mismatch", C.c_int32), ("reserved", C.c_int32 * 5)]


class CapReport(C.Structure):
    """adanerf_cap_report: what the sample cap did to the last render."""
    _fields_ = [("threshold_max", C.c_float), ("batches_trimmed", C.c_int32), ("samples_selected", C.c_int64), ("samples_kept", C.c_int64)]


EXPORTS = ["adanerf_create", "adanerf_destroy", "adanerf_get_info", "adanerf_last_error", "adanerf_abi_version", "adanerf_struct_sizes", "adanerf_set_camera", "adanerf_set_selection", "adanerf_set_frame_size", "adanerf_present", "adanerf_reproject",
           "adanerf_reproject_gather", "adanerf_reproject_pair", "adanerf_host_pair_weight",
           "adanerf_set_budget_map", "adanerf_foveate", "adanerf_compact_budget",
           "adanerf_render", "adanerf_set_aux_outputs", "adanerf_set_disp_output", "adanerf_assemble_strips", "adanerf_sync", "adanerf_set_stream", "adanerf_set_profiling",
           "adanerf_collect_stats", "adanerf_ray_features", "adanerf_sample_mlp",
           "adanerf_compact", "adanerf_compact_guarded", "adanerf_calibrate_guard", "adanerf_guard_calibration_file", "adanerf_shade_features", "adanerf_shade_mlp", "adanerf_shade_mlp_z", "adanerf_sample_pdf", "adanerf_sample_uniform", "adanerf_shade_mlp_coarse", "adanerf_sample_from_coarse",
           "adanerf_composite", "adanerf_composite_classic", "adanerf_composite_aux", "adanerf_composite_classic_aux", "adanerf_disp_map", "adanerf_copy_result_sampling_network", "adanerf_flip",
           "adanerf_render_oracle", "adanerf_gather_to", "adanerf_probe_mfma", "adanerf_malloc",
           "adanerf_free", "adanerf_memcpy_h2d", "adanerf_memcpy_d2h", "adanerf_get_buffer",
           "adanerf_set_pixel_offset", "adanerf_get_pixel_offset", "adanerf_accumulate", "adanerf_resolve_mean", "adanerf_host_subpixel_grid", "adanerf_temporal_resolve",
           "adanerf_temporal_upsample", "adanerf_render_masked",
           "adanerf_set_depth_limit", "adanerf_compact_depth_limit", "adanerf_blend_behind", "adanerf_host_sphere_zc",
           "adanerf_foveate_density", "adanerf_fill_density", "adanerf_host_density_mask",
           "adanerf_foveate_density_phased", "adanerf_fill_density_phased", "adanerf_host_density_mask_phased", "adanerf_host_density_phase",
           "adanerf_temporal_resolve_sparse",
           "adanerf_contrast_mask", "adanerf_accumulate_masked", "adanerf_resolve_mean_masked", "adanerf_host_contrast_mask",
           "adanerf_set_sample_cap", "adanerf_sample_cap_report", "adanerf_compact_cap"]

_lib = None


def load_library(path: Optional[str] = None):
    """dlopen libadanerf_hip.so (built in-tree by adanerf_amd.build).  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("ADANERF_LIB") or library_path()   # ADANERF_LIB: tools/ablate.sh variants
    if not os.path.exists(p):
        raise AdaNeRFError("HIP library not built: %s (run `python -c 'import __graft_entry__ as g; g.build()'`)" % p)
    lib = C.CDLL(p)
    vp, i32, f32p = C.c_void_p, C.c_int32, C.c_void_p
    lib.adanerf_create.argtypes = [C.c_char_p, C.POINTER(_Options), C.POINTER(vp)]
    lib.adanerf_destroy.argtypes = [vp]
    lib.adanerf_get_info.argtypes = [vp, C.POINTER(Info)]
    lib.adanerf_last_error.argtypes = [vp]
    lib.adanerf_last_error.restype = C.c_char_p
    lib.adanerf_set_camera.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.adanerf_set_selection.argtypes = [vp, i32, C.c_float]
    lib.adanerf_set_frame_size.argtypes = [vp, i32, i32]
    lib.adanerf_set_budget_map.argtypes = [vp, vp, vp]
    lib.adanerf_foveate.argtypes = [vp, C.c_float, C.c_float, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_float), vp, vp]
    lib.adanerf_compact_budget.argtypes = [vp, vp, i32, i32, C.c_float, vp, vp, vp, vp, vp, vp, vp]
    lib.adanerf_set_depth_limit.argtypes = [vp, vp]
    lib.adanerf_compact_depth_limit.argtypes = [vp, vp, i32, i32, C.c_float, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), vp, vp, vp, vp, vp]
    lib.adanerf_blend_behind.argtypes = [vp, vp, vp, vp, i32, vp, vp]
    lib.adanerf_set_sample_cap.argtypes = [vp, C.c_float]
    lib.adanerf_sample_cap_report.argtypes = [vp, C.POINTER(CapReport)]
    lib.adanerf_compact_cap.argtypes = [vp, vp, i32, i32, C.c_float, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64,
                                        vp, vp, vp, vp, vp, vp]
    lib.adanerf_host_sphere_zc.argtypes = [i32, i32, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float)]
    lib.adanerf_foveate_density.argtypes = [vp, C.c_float, C.c_float, i32, C.POINTER(i32), C.POINTER(i32), vp]
    lib.adanerf_fill_density.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, C.POINTER(i32)]
    lib.adanerf_host_density_mask.argtypes = [i32, i32, C.c_float, C.c_float, i32, C.POINTER(i32), C.POINTER(i32), vp]
    lib.adanerf_foveate_density_phased.argtypes = [vp, C.c_float, C.c_float, i32, C.POINTER(i32), C.POINTER(i32), i32, i32, vp]
    lib.adanerf_fill_density_phased.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, C.POINTER(i32)]
    lib.adanerf_host_density_mask_phased.argtypes = [i32, i32, C.c_float, C.c_float, i32, C.POINTER(i32), C.POINTER(i32), i32, i32, vp]
    lib.adanerf_host_density_phase.argtypes = [i32, C.POINTER(i32), C.POINTER(i32)]
    fp = C.POINTER(C.c_float)
    lib.adanerf_temporal_resolve_sparse.argtypes = [vp, vp, i32, i32, vp, vp, vp, fp, fp, vp, vp, vp, fp, fp, C.c_float, C.c_float, C.c_float, i32,
                                                    vp, vp, vp, vp, vp, C.POINTER(i32)]
    lib.adanerf_contrast_mask.argtypes = [vp, vp, i32, i32, C.c_float, vp, C.POINTER(i32)]
    lib.adanerf_accumulate_masked.argtypes = [vp, vp, vp, C.c_uint32, i32, vp, i32]
    lib.adanerf_resolve_mean_masked.argtypes = [vp, vp, vp, C.c_uint32, i32, i32, vp, vp]
    lib.adanerf_host_contrast_mask.argtypes = [vp, i32, i32, C.c_float, vp, C.POINTER(i32)]
    lib.adanerf_present.argtypes = [vp, vp, i32, i32, vp, i32, i32, i32]
    lib.adanerf_set_pixel_offset.argtypes = [vp, C.c_float, C.c_float]
    lib.adanerf_get_pixel_offset.argtypes = [vp, C.POINTER(C.c_float)]
    lib.adanerf_accumulate.argtypes = [vp, vp, i32, vp, i32]
    lib.adanerf_resolve_mean.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.adanerf_host_subpixel_grid.argtypes = [i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    fp = C.POINTER(C.c_float)
    lib.adanerf_reproject.argtypes = [vp, vp, vp, vp, fp, fp, fp, fp, C.c_float, C.c_uint32, i32, vp, vp, vp, C.POINTER(i32)]
    lib.adanerf_reproject_gather.argtypes = [vp, vp, vp, vp, fp, fp, fp, fp, C.c_float, C.c_float, i32, C.c_uint32, i32, vp, vp, vp, vp, C.POINTER(i32)]
    lib.adanerf_reproject_pair.argtypes = [vp, vp, vp, vp, fp, fp, vp, vp, vp, fp, fp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_uint32, i32,
                                           vp, vp, vp, vp, vp, C.POINTER(i32)]
    lib.adanerf_host_pair_weight.argtypes = [fp, fp, fp, fp]
    lib.adanerf_temporal_resolve.argtypes = [vp, vp, vp, vp, fp, fp, vp, vp, vp, fp, fp, C.c_float, C.c_float, C.c_float, i32, vp, vp, vp, vp, vp,
                                             C.POINTER(i32)]
    lib.adanerf_temporal_upsample.argtypes = [vp, i32, vp, vp, vp, C.c_float, C.c_float, fp, fp, vp, vp, vp, fp, fp, C.c_float, C.c_float, C.c_float, i32,
                                              vp, vp, vp, vp, vp, C.POINTER(i32)]
    lib.adanerf_render.argtypes = [vp, vp, vp, C.POINTER(Stats)]
    lib.adanerf_render_masked.argtypes = [vp, vp, C.c_uint32, vp, vp, C.POINTER(Stats), C.POINTER(i32)]
    lib.adanerf_assemble_strips.argtypes = [vp, vp, vp]
    lib.adanerf_set_aux_outputs.argtypes = [vp, vp, vp]
    lib.adanerf_set_disp_output.argtypes = [vp, vp]
    lib.adanerf_sync.argtypes = [vp]
    lib.adanerf_set_stream.argtypes = [vp, vp]
    lib.adanerf_set_profiling.argtypes = [vp, i32]
    lib.adanerf_collect_stats.argtypes = [vp, C.POINTER(Stats), C.POINTER(i32)]
    lib.adanerf_ray_features.argtypes = [vp, i32, i32, f32p, f32p]
    lib.adanerf_sample_mlp.argtypes = [vp, i32, i32, f32p, f32p]
    lib.adanerf_compact.argtypes = [vp, vp, i32, i32, C.c_float, vp, vp, vp, vp, vp]
    lib.adanerf_compact_guarded.argtypes = [vp, vp, vp, i32, i32, C.c_float, C.c_float, C.c_float, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.adanerf_calibrate_guard.argtypes = [vp, i32, C.c_uint32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.adanerf_guard_calibration_file.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.adanerf_abi_version.argtypes = []
    lib.adanerf_struct_sizes.argtypes = [C.POINTER(i32)]
    lib.adanerf_shade_features.argtypes = [vp, vp, vp, i32, vp]
    lib.adanerf_shade_mlp.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    lib.adanerf_composite.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp]
    lib.adanerf_shade_mlp_z.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    lib.adanerf_sample_pdf.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.adanerf_sample_uniform.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    lib.adanerf_shade_mlp_coarse.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    lib.adanerf_sample_from_coarse.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.adanerf_composite_classic.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp]
    lib.adanerf_composite_aux.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.adanerf_composite_classic_aux.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.adanerf_disp_map.argtypes = [vp, vp, vp, i32, vp]
    lib.adanerf_copy_result_sampling_network.argtypes = [vp, vp, i32, vp]
    lib.adanerf_flip.argtypes = [vp, vp, vp, i32, i32, C.c_float, vp, C.POINTER(C.c_float)]
    lib.adanerf_render_oracle.argtypes = [vp, vp]
    lib.adanerf_gather_to.argtypes = [vp, vp, vp, vp, C.c_size_t]
    lib.adanerf_probe_mfma.argtypes = [vp, i32, i32, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.adanerf_malloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.adanerf_free.argtypes = [vp, vp]
    lib.adanerf_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    lib.adanerf_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    lib.adanerf_get_buffer.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    for name in EXPORTS:
        if name != "adanerf_last_error":
            getattr(lib, name).restype = C.c_int
    # the handshake include/adanerf_hip.h asks of a binding: structs are written whole, so version and sizes must agree
    sizes = (i32 * 3)()
    lib.adanerf_struct_sizes(sizes)
    if lib.adanerf_abi_version() != ABI_VERSION or list(sizes) != [C.sizeof(_Options), C.sizeof(Info), C.sizeof(Stats)]:
        raise AdaNeRFError("%s: ABI %d with struct sizes %s, this host expects ABI %d with %s" %
                           (p, lib.adanerf_abi_version(), list(sizes), ABI_VERSION, [C.sizeof(_Options), C.sizeof(Info), C.sizeof(Stats)]))
    if path is None:
        _lib = lib
    return lib


@dataclass
class Settings:
    """Viewer CLI settings (adanerf_real_time_viewer/src/settings.cpp:15-47)."""
    model_path: str
    width: int = 800
    height: int = 800
    batch_size: int = -1          # -bs: <= 0 -> width*height, else min(bs, w*h)
    number_of_batches: int = 1    # -nb (overridden by batch_size)
    write_images: bool = False
    is_debug: bool = True         # headless always
    window_width: Optional[int] = None    # -ws: the size a frame is presented at (NeuralRenderer.present); None -> the frame size
    window_height: Optional[int] = None   # at construction, as the viewer's Settings defaults it

    def __post_init__(self):
        if self.window_width is None:
            self.window_width = self.width
        if self.window_height is None:
            self.window_height = self.height

    @property
    def total_size(self) -> int:
        return self.width * self.height

    def requested_batch(self) -> int:
        """What adanerf_options.batch_rays gets: -bs as given (the library clamps it to the frame, again at every set_frame_size), -nb's
        share of the first frame, 0 for the whole frame."""
        if self.batch_size and self.batch_size > 0:
            return int(self.batch_size)
        return self.resolved_batch() if self.number_of_batches > 1 else 0

    def resolved_batch(self) -> int:
        if self.batch_size and self.batch_size > 0:
            return min(self.batch_size, self.total_size)
        if self.number_of_batches > 1:
            return -(-self.total_size // self.number_of_batches)
        return self.total_size


class DeviceArray:
    """A device allocation owned by the library's allocator, with numpy round trips."""

    def __init__(self, r: "NeuralRenderer", shape, dtype):
        self.r = r
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        r._check(r.lib.adanerf_malloc(r.handle, max(self.nbytes, 1), C.byref(p)))
        self.ptr = p.value

    def upload(self, arr: np.ndarray) -> "DeviceArray":
        a = np.ascontiguousarray(arr, dtype=self.dtype)
        assert a.nbytes == self.nbytes, (a.shape, self.shape)
        if self.nbytes:
            self.r._check(self.r.lib.adanerf_memcpy_h2d(self.r.handle, self.ptr, a.ctypes.data, self.nbytes))
        return self

    def numpy(self, count: Optional[int] = None) -> np.ndarray:
        shape = self.shape if count is None else (count,) + self.shape[1:]
        out = np.empty(shape, dtype=self.dtype)
        if out.nbytes:
            self.r._check(self.r.lib.adanerf_memcpy_d2h(self.r.handle, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr and self.r.handle:
            self.r.lib.adanerf_free(self.r.handle, self.ptr)
        self.ptr = None


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, DeviceArray):
        return x.ptr
    if hasattr(x, "data_ptr"):      # torch tensor on the context's device
        return x.data_ptr()
    return int(x)


def _pose_ptrs(*arrays):
    """(pos, rot, pos, rot, ...) -> their C float pointers ([3] and [9] fp32, contiguous); None stays None.  A pointer keeps its array alive."""
    f = [None if v is None else np.ascontiguousarray(v, dtype=np.float32).reshape(9 if i % 2 else 3) for i, v in enumerate(arrays)]
    return [None if v is None else v.ctypes.data_as(C.POINTER(C.c_float)) for v in f]


def _release(owner, arrays):
    """Frees device arrays ``owner`` made with empty(): off its list, and ``_last_frame`` cleared if it showed one of them."""
    for a in arrays:
        if owner._last_frame is not None and owner._last_frame[0] is a:
            owner._last_frame = None
        a.free()
        owner._own.remove(a)


def _check_blend(who: str, alpha, depth_tol):
    """alpha / depth_tol of a temporal stage as floats; ValueError outside (0, 1] / below 0 (a NaN fails both)."""
    if not 0.0 < float(alpha) <= 1.0:
        raise ValueError("%s: alpha must lie in (0, 1], got %r" % (who, alpha))
    if not float(depth_tol) >= 0.0:
        raise ValueError("%s: depth_tol must be >= 0, got %r" % (who, depth_tol))
    return float(alpha), float(depth_tol)


class _History:
    """What a temporal stage keeps on the device between frames: two sets (rgb [n,3] fp32, depth [n] fp32, count [n] uint8) that ping-pong,
    which one was written last and at which pose -- ``hist`` = (index into ``sets``, pos, rot), None without a history -- and the stage's
    other buffers of the same pixel count, ``extras`` = ((attribute, columns, dtype), ...).  ``owner`` makes them (empty()) and lists them
    (_own, _last_frame: see _release)."""

    def __init__(self, owner, extras=()):
        self.owner, self.extras = owner, tuple(extras)
        self.n, self.sets, self.hist = None, [], None

    def buffers(self):
        return [] if self.n is None else [b for st in self.sets for b in st] + [getattr(self, name) for name, _, _ in self.extras]

    def ensure(self, n: int):
        """Everything for n pixels: made on first use and again, without a history, when n changes."""
        if self.n == n:
            return
        _release(self.owner, self.buffers())
        e = self.owner.empty
        self.sets = [(e((n, 3), np.float32), e((n,), np.float32), e((n,), np.uint8)) for _ in range(2)]
        for name, cols, dtype in self.extras:
            setattr(self, name, e((n, cols) if cols > 1 else (n,), dtype))
        self.n, self.hist = n, None

    def _out(self) -> int:
        return 0 if self.hist is None else 1 - self.hist[0]

    def inputs(self, pose):
        """For a resolve at ``pose`` = (pos, rot): (hist_rgb, hist_depth, hist_count, prev_pos, prev_rot, out_set), Nones without a
        history.  The camera has not moved since the history was written: in a static scene nothing can have been uncovered, so there is
        no disocclusion test (hist_depth None).  The test would compare the depths of two jittered renders of one pose, and where a pixel
        spans several surfaces the jitter alone moves its depth past any tolerance: those pixels would restart their mean for nothing."""
        out = self.sets[self._out()]
        if self.hist is None:
            return None, None, None, None, None, out
        side, pos, rot = self.hist
        rgb, depth, count = self.sets[side]
        at_rest = np.array_equal(pos, pose[0]) and np.array_equal(rot, pose[1])
        return rgb, None if at_rest else depth, count, pos, rot, out

    def commit(self, pose):
        """The resolve at ``pose`` has written inputs()'s out_set: it is the history now."""
        self.hist = (self._out(), pose[0], pose[1])

    def reset(self):
        """A cut: the next frame has no history.  The buffers stay."""
        self.hist = None


FOVEA_MAX_RINGS = 8


def pair_weight(dst_pos, a_pos, b_pos) -> float:
    """The weight_b of adanerf_reproject_pair for a destination between the keyframes at a_pos and b_pos (adanerf_host_pair_weight): its
    distance from A over the sum of its distances from A and B, 0.5 where both are 0 (a pure rotation).  No device needed.  ValueError on
    a position that is not finite."""
    fp = _pose_ptrs(dst_pos, None, a_pos, None, b_pos, None)
    out = C.c_float(0)
    if load_library().adanerf_host_pair_weight(fp[0], fp[2], fp[4], C.byref(out)) != 0:
        raise ValueError("adanerf_host_pair_weight(%r, %r, %r) refused: every value must be finite" % (dst_pos, a_pos, b_pos))
    return float(out.value)


def subpixel_grid(s: int):
    """The regular s x s sub-pixel pattern (adanerf_host_subpixel_grid): [(dx, dy)] * s*s in pixels, row by row, each a float that fp32
    holds exactly; s in 1..8, s = 1 gives [(0, 0)].  No device needed.  ValueError on anything else."""
    if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 1 <= s <= SUPERSAMPLE_MAX:
        raise ValueError("supersample: S must be an integer in 1..%d, got %r" % (SUPERSAMPLE_MAX, s))
    lib = load_library()
    out = []
    for k in range(int(s) * int(s)):
        dx, dy = C.c_float(0), C.c_float(0)
        if lib.adanerf_host_subpixel_grid(int(s), k, C.byref(dx), C.byref(dy)) != 0:
            raise AdaNeRFError("adanerf_host_subpixel_grid(%d, %d) failed" % (s, k))
        out.append((float(dx.value), float(dy.value)))
    return out


def sphere_zc(width: int, height: int, focal: float, pos, rot_c2w, center, radius: float) -> np.ndarray:
    """The camera-space depth of a sphere for every pixel of a width x height frame (adanerf_host_sphere_zc): [height*width] fp32, +inf
    where the pixel's ray misses it -- an occluder for set_depth_limit / render_hybrid without a rasteriser.  ``focal``: Info.focal.  No
    device needed.  ValueError on what the library refuses (a side outside 1..16384, a value that is not finite, radius <= 0)."""
    lib = load_library()
    fp = C.POINTER(C.c_float)
    p = np.ascontiguousarray(pos, dtype=np.float32).reshape(3)
    r = np.ascontiguousarray(rot_c2w, dtype=np.float32).reshape(9)
    c = np.ascontiguousarray(center, dtype=np.float32).reshape(3)
    ok = 1 <= int(width) <= 16384 and 1 <= int(height) <= 16384
    out = np.empty(int(width) * int(height) if ok else 1, dtype=np.float32)
    if lib.adanerf_host_sphere_zc(int(width), int(height), float(focal), p.ctypes.data_as(fp), r.ctypes.data_as(fp), c.ctypes.data_as(fp), float(radius),
                                  out.ctypes.data_as(fp)) != 0:
        raise ValueError("adanerf_host_sphere_zc(%r x %r, focal %r, radius %r) refused: sides in 1..16384, finite values, radius > 0" %
                         (width, height, focal, radius))
    return out


def parse_fovea(spec: str):
    """``R:N:T[,R:N:T...],N:T`` -> [(R, N, T), ..., (N, T)]: concentric rings around the gaze (radius in whole pixels, strictly ascending,
    at most 8), each with the sample budget N (0..255, 0 = the context's) and the threshold T of the pixels inside it, then the entry of
    the pixels outside every ring.  The form adanerf_foveate / NeuralRenderer.foveate take.  ValueError on anything else."""
    parts = [p.strip() for p in str(spec).split(",")]
    if not parts or any(not p for p in parts):
        raise ValueError("fovea %r: expected R:N:T[,R:N:T...],N:T" % (spec,))
    out = []
    for k, p in enumerate(parts):
        f = p.split(":")
        last = k == len(parts) - 1
        if len(f) != (2 if last else 3):
            raise ValueError("fovea %r: %r must be %s" % (spec, p, "N:T (the outside entry comes last)" if last else "R:N:T"))
        try:
            ints = [int(v) for v in f[:-1]]
            t = float(f[-1])
        except ValueError:
            raise ValueError("fovea %r: %r is not %s" % (spec, p, "N:T" if last else "R:N:T")) from None
        if t != t:
            raise ValueError("fovea %r: a threshold is not a number" % (spec,))
        if not 0 <= ints[-1] <= 255:
            raise ValueError("fovea %r: N must be in 0..255" % (spec,))
        if not last and (ints[0] < 0 or ints[0] >= 1 << 31 or (out and ints[0] <= out[-1][0])):
            raise ValueError("fovea %r: radii must be >= 0 and strictly ascending" % (spec,))
        out.append(tuple(ints) + (t,))
    if len(out) - 1 > FOVEA_MAX_RINGS:
        raise ValueError("fovea %r: at most %d rings" % (spec, FOVEA_MAX_RINGS))
    return out


DENSITY_STRIDES = (1, 2, 4, 8)


def parse_fovea_density(spec: str):
    """``R:S[,R:S...],S`` -> [(R, S), ..., (S,)]: concentric rings around the gaze (radius in whole pixels, strictly ascending, at most 8),
    each with the stride S (1, 2, 4 or 8: every S-th pixel per axis is rendered) of the pixels inside it, then the stride of the pixels
    outside every ring; strides never decrease outward.  The form adanerf_foveate_density / NeuralRenderer.foveate_density take.
    ValueError on anything else."""
    parts = [p.strip() for p in str(spec).split(",")]
    if not parts or any(not p for p in parts):
        raise ValueError("fovea density %r: expected R:S[,R:S...],S" % (spec,))
    out = []
    for k, p in enumerate(parts):
        f = p.split(":")
        last = k == len(parts) - 1
        if len(f) != (1 if last else 2):
            raise ValueError("fovea density %r: %r must be %s" % (spec, p, "S (the outside stride comes last)" if last else "R:S"))
        try:
            ints = [int(v) for v in f]
        except ValueError:
            raise ValueError("fovea density %r: %r is not %s" % (spec, p, "S" if last else "R:S")) from None
        if ints[-1] not in DENSITY_STRIDES:
            raise ValueError("fovea density %r: a stride must be 1, 2, 4 or 8" % (spec,))
        if out and ints[-1] < out[-1][-1]:
            raise ValueError("fovea density %r: strides must not decrease outward" % (spec,))
        if not last and (ints[0] < 0 or ints[0] >= 1 << 31 or (out and ints[0] <= out[-1][0])):
            raise ValueError("fovea density %r: radii must be >= 0 and strictly ascending" % (spec,))
        out.append(tuple(ints))
    if len(out) - 1 > FOVEA_MAX_RINGS:
        raise ValueError("fovea density %r: at most %d rings" % (spec, FOVEA_MAX_RINGS))
    return out


def _density_arrays(rings):
    rings = [tuple(r) for r in rings]
    nr = len(rings) - 1
    radius = (C.c_int32 * max(nr, 1))(*[int(r[0]) for r in rings[:-1]])
    stride = (C.c_int32 * (nr + 1))(*[int(r[-1]) for r in rings])
    return nr, radius, stride


def density_mask(width: int, height: int, gaze_xy, rings) -> np.ndarray:
    """The mask of adanerf_foveate_density on the host (adanerf_host_density_mask): [height*width] uint8, 0 = rendered, else the pixel's
    stride.  ``rings`` as parse_fovea_density returns them, or its string.  No device needed.  ValueError on what the library refuses."""
    if isinstance(rings, str):
        rings = parse_fovea_density(rings)
    nr, radius, stride = _density_arrays(rings)
    ok = 1 <= int(width) <= 16384 and 1 <= int(height) <= 16384
    out = np.empty(int(width) * int(height) if ok else 1, dtype=np.uint8)
    if load_library().adanerf_host_density_mask(int(width), int(height), float(gaze_xy[0]), float(gaze_xy[1]), nr, radius, stride, out.ctypes.data) != 0:
        raise ValueError("adanerf_host_density_mask(%r x %r, gaze %r, %r) refused" % (width, height, tuple(gaze_xy), rings))
    return out


def density_phase(k: int):
    """(phase_x, phase_y) of frame k of the lattice's 64-phase cycle (adanerf_host_density_phase): any L * L consecutive frames put
    every residue pair mod L on the lattice of level L exactly once, for L = 2, 4 and 8 at the same time."""
    px, py = C.c_int32(-1), C.c_int32(-1)
    k = ((int(k) + (1 << 31)) % (1 << 32)) - (1 << 31)      # as an int32; the cycle only reads k mod 64
    if load_library().adanerf_host_density_phase(k, C.byref(px), C.byref(py)) != 0:
        raise ValueError("adanerf_host_density_phase(%r) refused" % (k,))
    return int(px.value), int(py.value)


def density_mask_phased(width: int, height: int, gaze_xy, rings, phase_xy) -> np.ndarray:
    """density_mask with the lattice at phase (phase_x, phase_y), each 0..7 (adanerf_host_density_mask_phased); phase (0, 0) is
    density_mask.  ValueError on what the library refuses."""
    if isinstance(rings, str):
        rings = parse_fovea_density(rings)
    nr, radius, stride = _density_arrays(rings)
    ok = 1 <= int(width) <= 16384 and 1 <= int(height) <= 16384
    out = np.empty(int(width) * int(height) if ok else 1, dtype=np.uint8)
    if load_library().adanerf_host_density_mask_phased(int(width), int(height), float(gaze_xy[0]), float(gaze_xy[1]), nr, radius, stride,
                                                       int(phase_xy[0]), int(phase_xy[1]), out.ctypes.data) != 0:
        raise ValueError("adanerf_host_density_mask_phased(%r x %r, gaze %r, %r, phase %r) refused" % (width, height, tuple(gaze_xy), rings, tuple(phase_xy)))
    return out


def host_contrast_mask(rgb, width: int, height: int, threshold: float):
    """The mask of adanerf_contrast_mask on the host (adanerf_host_contrast_mask): ``rgb`` [height*width,3] fp32 -> (mask [height*width]
    uint8, 0 = flagged: a neighbour's display value differs by more than ``threshold`` in some channel; n_flagged).  No device needed.
    ValueError on what the library refuses (a side outside 1..16384, a threshold that is not finite or outside [0, 1])."""
    ok = 1 <= int(width) <= 16384 and 1 <= int(height) <= 16384
    a = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1)
    if ok and a.size != 3 * int(width) * int(height):
        raise ValueError("host_contrast_mask: %d values for a %d x %d image" % (a.size, width, height))
    out = np.empty(int(width) * int(height) if ok else 1, dtype=np.uint8)
    n = C.c_int32(0)
    if load_library().adanerf_host_contrast_mask(a.ctypes.data, int(width), int(height), float(threshold), out.ctypes.data, C.byref(n)) != 0:
        raise ValueError("adanerf_host_contrast_mask(%r x %r, threshold %r) refused" % (width, height, threshold))
    return out, int(n.value)


def choose_sampling(settings, pos=None, rot_c2w=None, precision="bf16", frames: int = 6, warmup: int = 2, margin: float = DEFAULT_RULE_MARGIN, **kw):
    """The default rule per workload: renders `frames` frames of this model / frame size / threshold in the split mode (exact by construction) and in
    the guarded mode (same frames while its measured band holds) and returns ("guarded" | "split", record): guarded only if it is >= margin faster
    here.  pos / rot_c2w: the camera to measure with (default: view-cell centre, looking down -z).  A configuration the guarded mode does not
    exist for (N > 16, run-time-shaped sampling networks, fp32) yields "split"."""
    import time
    fps, note = {}, None
    for mode in ("split", "guarded"):
        try:
            with NeuralRenderer(settings, precision=precision, sampling=mode, **kw) as r:
                p = np.asarray(pos if pos is not None else list(r.info.view_cell_center), np.float32)
                m = np.asarray(rot_c2w if rot_c2w is not None else np.eye(3), np.float32)
                r.set_camera(p, m)
                out = r.empty((r.info.rays_local, 4), np.uint8)
                for _ in range(warmup):
                    r.render(out, None)
                r.sync()
                t0 = time.perf_counter()
                for _ in range(frames):
                    r.render(out, None)
                r.sync()
                fps[mode] = frames / (time.perf_counter() - t0)
        except AdaNeRFError as e:
            if mode == "split":
                raise
            note = "guarded mode not available: %s" % e
    ahead = (fps["guarded"] / fps["split"] - 1.0) if "guarded" in fps else None
    choice = "guarded" if (ahead is not None and ahead >= margin) else "split"
    return choice, {"choice": choice, "split_fps": fps.get("split"), "guarded_fps": fps.get("guarded"), "guarded_ahead": ahead, "margin": margin,
                    "frames": frames, "note": note}


class NeuralRenderer:
    """Headless counterpart of the viewer's NeuralRenderer: ``init()`` loads the model directory and
    builds the device state, ``render()`` produces one frame."""

    def __init__(self, settings: Settings, precision="bf16", device_id: int = 0, num_samples: int = 0,
                 threshold: float = -1.0, shard_rank: int = 0, shard_world: int = 1, strip_rows: int = 8,
                 sampling: Optional[str] = None, lib_path: Optional[str] = None, keep_oracle: bool = False, wave_select: bool = False,
                 guard_eps: float = 0.0, guard_eps_pair: float = 0.0, guard_audit_period: int = 0, guard_cache: bool = True,
                 guard_audit_fill: bool = True):
        """sampling: arithmetic of the sampling network -- "split" (default: split-fp16, fp32-accurate on every ray, the selection exact by
        construction), "fp32" (fp32 MFMA), "guarded" (opt-in: plain fp16 for every ray + the split engine where the audited guard band cannot
        decide; the split engine's selections as long as the measured band holds -- monitored, audited, widened when violated), "fp16" (opt-in
        speed mode, the viewer's TensorRT arithmetic; selections differ on ~1 % of rays).  The default follows a rule: the mode that is
        exact by construction, unless the guarded mode is >= 8 % faster on the same box in the same bench.py run -- measured 4-5 %.  Same default in
        the `adanerf` CLI and bench.py.  guard_*: include/adanerf_hip.h adanerf_options.  guard_audit_fill (default): the audit fills the
        refinement pass's last round instead of adding one, and never audits less than a quarter of the 1 / period quota
        (ADANERF_FLAG_GUARD_AUDIT_FILL); False: exactly 1 / period of all rays every frame."""
        if sampling is None:
            sampling = "split"
        self.sampling_choice = None
        if sampling == "auto":      # the default rule applied to this model / frame size / threshold on this box, camera at the view-cell centre
            if precision == "fp32" or _PREC.get(precision, precision) == _PREC["fp32"]:
                sampling = "split"
            else:
                sampling, self.sampling_choice = choose_sampling(settings, precision=precision, device_id=device_id, num_samples=num_samples, threshold=threshold,
                                                                 shard_rank=shard_rank, shard_world=shard_world, strip_rows=strip_rows, lib_path=lib_path)
        self.settings = settings
        self.lib = load_library(lib_path)
        self.handle = None
        self._opt = _Options(width=settings.width, height=settings.height, batch_rays=settings.requested_batch(),
                             device_id=device_id, precision=_PREC[precision] if isinstance(precision, str) else int(precision),
                             num_samples=num_samples, threshold=threshold, shard_rank=shard_rank,
                             shard_world=shard_world, strip_rows=strip_rows,
                             sampling_mode=SAMPLING_MODES[sampling], guard_eps=guard_eps, guard_eps_pair=guard_eps_pair,
                             guard_audit_period=guard_audit_period,
                             flags=(FLAG_KEEP_ORACLE if keep_oracle else 0) | (FLAG_WAVE_SELECT if wave_select else 0) |
                                   (0 if guard_cache else FLAG_NO_GUARD_CACHE) | (FLAG_GUARD_AUDIT_FILL if guard_audit_fill else 0))
        self.info = Info()
        self.last_stats = Stats()
        self._own = []
        self._last_frame = None       # (device rgba8, width, height) of the last render() that wrote one
        self._pose = None             # (pos [3], rot [9]) of the last set_camera
        self._rp_on = False           # enable_reprojection(): render_numpy keeps depth, acc and the pose of its frame
        self._rp_frame = None         # (device rgba8, depth, acc, pos, rot, rays) of the last render_numpy since then
        self._ip_on = False           # enable_interpolation(): render_keyframe keeps two frames for interpolate()
        self._ip_keys = []            # [(set 0 / 1, pos, rot)] of the keyframes kept, the older first
        self._ta = None               # enable_temporal(): alpha, depth_tol, clamp, the cycle of sub-pixel offsets and the place in it
        self._ta_history = _History(self, [("mask", 1, np.uint8)])      # render_temporal's history and verdict mask
        self._tu = None               # enable_temporal_upsample(): scale, alpha, depth_tol, clamp, the offset cycle and the place in it
        self._tu_history = _History(self, [("mask", 1, np.uint8), ("rgba", 4, np.uint8)])      # render_upsampled's, at the output size, and its 8-bit image
        self._ft = None               # enable_foveated_temporal(): alpha, depth_tol, clamp and the frame number k of the phase cycle
        # render_foveated_temporal's, and the density mask of the phase (render_foveated's own mask stays at phase (0, 0))
        self._ft_history = _History(self, [("mask", 1, np.uint8), ("rgba", 4, np.uint8), ("dmask", 1, np.uint8)])
        # device buffers of the renderer's own, made on first use by _buffers() and dropped by _drop_buffers(): render_numpy's outputs, the
        # budget maps, the aux outputs and warp images of reproject(), the density mask, the depth limit, the sums and masks of the supersamplers
        for name in ("_o_rgb", "_o_rgba", "_b_n", "_b_thr", "_rp_depth", "_rp_acc", "_rp_rgba", "_rp_mask", "_rp_rgb", "_rp_wrgb", "_ip_rgb0", "_ip_depth0", "_ip_acc0", "_ip_rgb1", "_ip_depth1", "_ip_acc1", "_ip_wrgb", "_ip_rgba", "_ip_mask",
                     "_ip_source", "_fd_mask", "_dl_buf",
                     "_hy_acc", "_hy_behind", "_hy_limit", "_ss_sum", "_sa_stage", "_sa_mask"):
            setattr(self, name, None)
        self._dl_in_force = None      # what the last set_depth_limit installed; render_hybrid puts it back
        self._aux_in_force = (None, None)   # (depth_map, acc_map) of the last set_aux_outputs, likewise
        self._disp_in_force = None    # the disp_map of the last set_disp_output; render_supersampled_adaptive puts it back
        self._fd = None               # foveate_density(): (gaze, rings, width, height) the device mask _fd_mask was filled for

    # -- lifecycle -------------------------------------------------------------------------------
    def init(self) -> bool:
        h = C.c_void_p()
        rc = self.lib.adanerf_create(self.settings.model_path.encode(), C.byref(self._opt), C.byref(h))
        if rc != 0:
            raise AdaNeRFError("adanerf_create(%s) failed (%d): %s" %
                               (self.settings.model_path, rc, self.lib.adanerf_last_error(None).decode()))
        self.handle = h.value
        self._check(self.lib.adanerf_get_info(self.handle, C.byref(self.info)))
        return True

    def close(self):
        if self.handle:
            for a in self._own:
                a.free()
            self._own = []
            self.lib.adanerf_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        if not self.handle:
            self.init()
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            msg = self.lib.adanerf_last_error(self.handle).decode() if self.handle else "?"
            raise AdaNeRFError("libadanerf_hip error %d: %s" % (rc, msg))

    def empty(self, shape, dtype) -> DeviceArray:
        a = DeviceArray(self, shape, dtype)
        self._own.append(a)
        return a

    def to_device(self, arr: np.ndarray) -> DeviceArray:
        return self.empty(arr.shape, arr.dtype).upload(arr)

    def _buffers(self, *specs) -> bool:
        """The renderer's own device buffers ``specs`` = (attribute, shape, dtype), ...: made on first use, and made again -- all of them,
        and True returned -- when the shape of the first has changed."""
        a = getattr(self, specs[0][0])
        if a is not None and a.shape == specs[0][1]:
            return False
        self._drop_buffers(*[name for name, _, _ in specs])
        for name, shape, dtype in specs:
            setattr(self, name, self.empty(shape, dtype))
        return True

    def _drop_buffers(self, *names):
        _release(self, [getattr(self, name) for name in names if getattr(self, name) is not None])
        for name in names:
            setattr(self, name, None)

    def _out_buffers(self):
        """``_o_rgb`` / ``_o_rgba``: the fp32 and 8-bit frame of the render size in force"""
        n = self.info.rays_local
        self._buffers(("_o_rgb", (n, 3), np.float32), ("_o_rgba", (n, 4), np.uint8))

    # -- per frame ---------------------------------------------------------------------------------
    def set_camera(self, pos, rot_c2w):
        p = np.ascontiguousarray(pos, dtype=np.float32).reshape(3)
        r = np.ascontiguousarray(rot_c2w, dtype=np.float32).reshape(9)
        self._check(self.lib.adanerf_set_camera(self.handle, p.ctypes.data_as(C.POINTER(C.c_float)),
                                                r.ctypes.data_as(C.POINTER(C.c_float))))
        self._pose = (p.copy(), r.copy())

    def set_selection(self, num_samples: Optional[int] = None, threshold: Optional[float] = None) -> "Info":
        """The sample budget N and / or the selection threshold for the frames rendered from now on (None keeps the one in force); the
        context is then what one constructed with these values would be, without reloading the model (adanerf_set_selection).
        threshold 0 is the dense mode and needs num_samples 128.  Refreshes and returns ``self.info``.  A ``sampling="auto"`` choice made
        at construction is not re-measured: the mode chosen for the first pair stays."""
        self._check(self.lib.adanerf_set_selection(self.handle, 0 if num_samples is None else int(num_samples),
                                                   -1.0 if threshold is None else float(threshold)))
        return self.refresh_info()

    def set_frame_size(self, width: Optional[int] = None, height: Optional[int] = None) -> "Info":
        """The frame size for the frames rendered from now on (None keeps the value in force); the context is then what one constructed
        with this size would be, without reloading the model (adanerf_set_frame_size).  ``settings.width / height`` follow, the window
        size stays; the renderer's own output buffers (render_numpy) are made again at the next frame; device buffers the caller made
        for the old size, the ones behind set_aux_outputs / set_disp_output included (the library drops those when rays_local
        changes), are the caller's to re-make.  Refreshes and returns ``self.info``."""
        was_rays = self.info.rays_local
        self._check(self.lib.adanerf_set_frame_size(self.handle, 0 if width is None else int(width), 0 if height is None else int(height)))
        self.refresh_info()
        if self.info.rays_local != was_rays:      # the library dropped the per-ray buffers of the old rays_local
            self._dl_in_force, self._aux_in_force, self._disp_in_force = None, (None, None), None
        self.settings.width, self.settings.height = self.info.width, self.info.height
        if self._b_n is not None and self._b_n.shape[0] != self.info.rays_local:      # the library dropped the maps with the old rays_local
            self._drop_buffers("_b_n", "_b_thr")
        self._rp_frame = None      # a frame of the old size cannot be warped with the new size's ray generator
        self._ip_keys = []         # nor can keyframes of the old size
        for history in (self._ta_history, self._tu_history, self._ft_history):      # nor can a history of the old size be gathered from
            history.reset()
        self._fd = None            # the density mask is per frame size: foveate_density() fills it again
        self._drop_buffers("_o_rgb", "_o_rgba")
        return self.info

    # -- per-ray sample budgets ----------------------------------------------------------------------
    def budget_buffers(self):
        """The renderer's own device maps ([rays_local] uint8 N, [rays_local] fp32 threshold), made on first use and again after a frame
        size that changes rays_local.  Fill them (upload, foveate_device) and install them with set_budget_map."""
        n = self.info.rays_local
        self._buffers(("_b_n", (n,), np.uint8), ("_b_thr", (n,), np.float32))
        return self._b_n, self._b_thr

    def set_budget_map(self, n_map=None, thr_map=None):
        """Per-ray sample budgets for the frames rendered from now on (adanerf_set_budget_map): n_map [rays_local] uint8 (0 or above the
        context's N: the context's N), thr_map [rays_local] fp32 (not above the context's threshold: the context's).  Each is a numpy array
        (uploaded into the renderer's own buffer), a device buffer (the renderer's budget_buffers(), a DeviceArray, a pointer) or None (that
        half follows the context); both None turns the feature off.  A frame size that changes rays_local removes the maps."""
        own = self.budget_buffers() if any(isinstance(m, np.ndarray) for m in (n_map, thr_map)) else (None, None)
        ptrs = []
        for m, buf, dt in ((n_map, own[0], np.uint8), (thr_map, own[1], np.float32)):
            if isinstance(m, np.ndarray):
                if m.size != self.info.rays_local:
                    raise ValueError("set_budget_map: %d entries for %d local rays" % (m.size, self.info.rays_local))
                self.sync()      # frames in flight still read the buffer
                buf.upload(m.reshape(-1).astype(dt, copy=False))
                m = buf
            ptrs.append(_ptr(m))
        self._check(self.lib.adanerf_set_budget_map(self.handle, ptrs[0], ptrs[1]))

    def set_sample_cap(self, mean: float = 0.0):
        """A hard upper bound on the samples of the frames rendered from now on (adanerf_set_sample_cap): a batch of n rays shades at most
        floor(mean * n) samples; the threshold is raised on the device, in the same frame, by exactly as much as that needs.  0 removes the
        cap; otherwise ``mean`` is finite and >= 1.  Survives set_selection and set_frame_size."""
        self._check(self.lib.adanerf_set_sample_cap(self.handle, float(mean)))

    def sample_cap_report(self) -> CapReport:
        """What the cap did to the last render (adanerf_sample_cap_report; synchronises once): threshold_max (-inf: no batch was trimmed),
        batches_trimmed, samples_selected, samples_kept."""
        rep = CapReport()
        self._check(self.lib.adanerf_sample_cap_report(self.handle, C.byref(rep)))
        return rep

    def foveate_device(self, gaze_xy, rings, n_map=None, thr_map=None) -> int:
        """adanerf_foveate into device buffers (either may be None): rings as parse_fovea returns them, [(R, N, T), ..., (N, T)].
        Returns the library's code (0, or ADANERF_EINVAL with nothing written) instead of raising: tests look at both."""
        rings = [tuple(r) for r in rings]
        nr = len(rings) - 1
        radius = (C.c_int32 * max(nr, 1))(*[int(r[0]) for r in rings[:-1]])
        n = (C.c_int32 * (nr + 1))(*[int(r[-2]) for r in rings])
        thr = (C.c_float * (nr + 1))(*[float(r[-1]) for r in rings])
        return self.lib.adanerf_foveate(self.handle, float(gaze_xy[0]), float(gaze_xy[1]), nr, radius, n, thr, _ptr(n_map), _ptr(thr_map))

    def foveate(self, gaze_xy, rings):
        """Foveated rendering from now on: fills the renderer's own maps from the gaze point (pixels) and the rings ([(R, N, T), ...,
        (N, T)] or the string parse_fovea takes) on the device, then installs them.  Call again when the gaze moves or the frame size
        changes; set_budget_map() removes them."""
        if isinstance(rings, str):
            rings = parse_fovea(rings)
        n_map, thr_map = self.budget_buffers()
        self._check(self.foveate_device(gaze_xy, rings, n_map, thr_map))
        self._check(self.lib.adanerf_set_budget_map(self.handle, n_map.ptr, thr_map.ptr))

    # -- foveated ray density: a mask of strides around the gaze, the pixels in between rebuilt ------------
    def foveate_density_device(self, gaze_xy, rings, mask) -> int:
        """adanerf_foveate_density into a device buffer ([height*width] uint8): rings as parse_fovea_density returns them, [(R, S), ...,
        (S,)].  Returns the library's code (0, or an error with nothing written) instead of raising: tests look at both."""
        nr, radius, stride = _density_arrays(rings)
        return self.lib.adanerf_foveate_density(self.handle, float(gaze_xy[0]), float(gaze_xy[1]), nr, radius, stride, _ptr(mask))

    def fill_density_device(self, mask, width: int, height: int, rgb, depth_map=None, acc_map=None, rgba8=None, count: bool = True):
        """adanerf_fill_density over device images, in place: every pixel whose mask byte is 2, 4 or 8 becomes the bilinear blend of the
        rendered corners of its cell.  Returns (code, unfilled); ``count=False`` passes no counter (asynchronous, unfilled is None)."""
        u = C.c_int32(-1)
        rc = self.lib.adanerf_fill_density(self.handle, _ptr(mask), int(width), int(height), _ptr(rgb), _ptr(depth_map), _ptr(acc_map), _ptr(rgba8),
                                           C.byref(u) if count else None)
        return rc, (int(u.value) if count else None)

    density_mask = staticmethod(density_mask)

    def foveate_density(self, gaze_xy, rings):
        """Foveated ray density from now on for render_foveated(): fills the renderer's own device mask from the gaze point (pixels) and
        the rings ([(R, S), ..., (S,)] or the string parse_fovea_density takes).  Call again when the gaze moves; a frame-size change
        drops the mask, so call again after set_frame_size too."""
        if isinstance(rings, str):
            rings = parse_fovea_density(rings)
        n = self.info.width * self.info.height
        if self._fd_mask is not None and self._fd_mask.shape[0] != n:
            self.sync()      # a frame in flight still reads the mask
        self._buffers(("_fd_mask", (n,), np.uint8))
        self._fd = None
        self._check(self.foveate_density_device(gaze_xy, rings, self._fd_mask))
        self._fd = ((float(gaze_xy[0]), float(gaze_xy[1])), [tuple(r) for r in rings], self.info.width, self.info.height)

    def render_foveated(self):
        """One frame at the density foveate_density() set: adanerf_render_masked over the mask's lattice into the renderer's own images,
        then adanerf_fill_density for the pixels in between -- colour, RGBA8 and the aux maps in force.  Returns (rgb [R,3] fp32, rgba8
        [R,4] uint8, rendered, Stats of the rendered rays); the device copies stay in ``_o_rgb`` / ``_o_rgba`` as after render_numpy."""
        w, h = self.info.width, self.info.height
        if self._fd is None or self._fd[2:] != (w, h):
            raise AdaNeRFError("render_foveated: no density mask for %d x %d (call foveate_density first, and again after set_frame_size)" % (w, h))
        n = self.info.rays_local
        self._out_buffers()
        rendered, st = self.render_masked(self._fd_mask, 1, self._o_rgba, self._o_rgb)
        rc, _ = self.fill_density_device(self._fd_mask, w, h, self._o_rgb, self._aux_in_force[0], self._aux_in_force[1], self._o_rgba, count=False)
        self._check(rc)
        self._last_frame = (self._o_rgba, w, h)
        self._rp_frame = None      # the depth between the rendered pixels is interpolated, not the volume's own
        return self._o_rgb.numpy(), self._o_rgba.numpy(), rendered, st

    # -- foveated density over time: the lattice moves through 64 phases, the sparse temporal resolve keeps what was rendered ----
    density_phase = staticmethod(density_phase)
    density_mask_phased = staticmethod(density_mask_phased)

    def foveate_density_phased_device(self, gaze_xy, rings, phase_xy, mask) -> int:
        """adanerf_foveate_density_phased into a device buffer: foveate_density_device with the lattice at phase (phase_x, phase_y).
        Returns the library's code instead of raising."""
        nr, radius, stride = _density_arrays(rings)
        return self.lib.adanerf_foveate_density_phased(self.handle, float(gaze_xy[0]), float(gaze_xy[1]), nr, radius, stride, int(phase_xy[0]),
                                                       int(phase_xy[1]), _ptr(mask))

    def fill_density_phased_device(self, mask, width: int, height: int, phase_xy, rgb, depth_map=None, acc_map=None, rgba8=None, count: bool = True):
        """adanerf_fill_density_phased over device images, in place: fill_density_device with the cells of the lattice at phase
        (phase_x, phase_y).  Returns (code, unfilled); ``count=False`` passes no counter (asynchronous, unfilled is None)."""
        u = C.c_int32(-1)
        rc = self.lib.adanerf_fill_density_phased(self.handle, _ptr(mask), int(width), int(height), int(phase_xy[0]), int(phase_xy[1]), _ptr(rgb),
                                                  _ptr(depth_map), _ptr(acc_map), _ptr(rgba8), C.byref(u) if count else None)
        return rc, (int(u.value) if count else None)

    def temporal_resolve_sparse_device(self, mask, phase_xy, cur_rgb, cur_depth, cur_acc, cur_pos, cur_rot, hist_rgb, hist_depth, hist_count, prev_pos,
                                       prev_rot, out_rgb, out_depth, out_count, out_rgba8=None, out_mask=None, alpha: float = 0.1,
                                       depth_tol: float = 0.02, acc_min: float = 0.5, clamp: bool = True, rejected: bool = True) -> Optional[int]:
        """adanerf_temporal_resolve_sparse on device images of the context's frame size: temporal_resolve_device told by ``mask`` (the
        frame's density mask, phase ``phase_xy``) which pixels were rendered (they refresh the history) and which the fill reconstructed
        (they keep the history they have).  out_count is required, and hist_count with a history.  out_mask: 1 the history was used, 2 it
        held only a placeholder, 0 rejected.  Returns the number of rejected pixels (synchronous); with rejected=False nothing is read
        back and the outputs are complete after sync()."""
        fp = _pose_ptrs(cur_pos, cur_rot, prev_pos, prev_rot)
        n = C.c_int32(0)
        self._check(self.lib.adanerf_temporal_resolve_sparse(self.handle, _ptr(mask), int(phase_xy[0]), int(phase_xy[1]), _ptr(cur_rgb), _ptr(cur_depth),
                                                             _ptr(cur_acc), fp[0], fp[1], _ptr(hist_rgb), _ptr(hist_depth), _ptr(hist_count), fp[2], fp[3],
                                                             float(alpha), float(depth_tol), float(acc_min), TEMPORAL_CLAMP if clamp else 0, _ptr(out_rgb),
                                                             _ptr(out_depth), _ptr(out_count), _ptr(out_rgba8), _ptr(out_mask),
                                                             C.byref(n) if rejected else None))
        return int(n.value) if rejected else None

    def enable_foveated_temporal(self, alpha: float = 0.1, depth_tol: float = 0.02, clamp: bool = True):
        """Foveated density over time from now on through render_foveated_temporal(): the lattice of foveate_density() -- which must have
        set the gaze and rings -- moves through the 64 phases of density_phase, and every frame is resolved against a history kept on the
        device (adanerf_temporal_resolve_sparse): rendered pixels refresh it, reconstructed pixels keep what they have.  alpha, depth_tol,
        clamp: as enable_temporal's (the depth test is over a rendered pixel's 3 x 3 neighbourhood, a reconstructed pixel's corners; the
        clamp applies to rendered pixels).  Whole frames of models without useNDC only.  The depth_map / acc_map aux outputs become the
        renderer's own."""
        if self.info.use_ndc or self.info.rays_local != self.info.width * self.info.height:
            raise AdaNeRFError("foveated density over time needs a whole frame of a model without useNDC")
        if self._fd is None:
            raise AdaNeRFError("enable_foveated_temporal: call foveate_density first (it sets the gaze and the rings)")
        alpha, depth_tol = _check_blend("enable_foveated_temporal", alpha, depth_tol)
        self._ft = dict(alpha=alpha, depth_tol=depth_tol, clamp=bool(clamp), k=0)
        self._temporal_buffers(self._ft_history, self.info.rays_local)
        self._ft_history.reset()

    def reset_foveated_temporal(self):
        """Drops the history (a cut): the next render_foveated_temporal shows its frame as render_foveated would at that phase.  The
        phase cycle goes on."""
        self._ft_history.reset()

    def render_foveated_temporal(self):
        """One frame at the camera of the last set_camera: frame k takes the phase density_phase(k), fills the mask of foveate_density()'s
        gaze and rings at that phase, renders its lattice (adanerf_render_masked), rebuilds the pixels in between
        (adanerf_fill_density_phased) and resolves the frame against the history, which it then replaces (two buffer sets ping-pong on the
        device).  Returns (rgb fp32 [R,3], rgba8 [R,4] uint8, mask [R] uint8, rejected, rendered, Stats of the rendered rays): mask 1
        where the history was used, 2 where it held only a placeholder; rejected counts mask 0 (every pixel on the first frame and after
        reset_foveated_temporal / set_frame_size).  While the pose is bit for bit the one of the call before, the history's depth is not
        tested (nothing is uncovered while the camera rests).  render_foveated() and its mask are untouched: the phased mask is a buffer
        of this path's own (``_ft_history.dmask``).  present() shows the resolved frame."""
        if self._ft is None:
            raise AdaNeRFError("render_foveated_temporal: call enable_foveated_temporal first")
        if self._pose is None:
            raise AdaNeRFError("render_foveated_temporal needs the pose of the frame: call set_camera first")
        w, h = self.info.width, self.info.height
        if self._fd is None or self._fd[2:] != (w, h):
            raise AdaNeRFError("render_foveated_temporal: no density mask for %d x %d (call foveate_density first, and again after set_frame_size)" % (w, h))
        ft, hi = self._ft, self._ft_history
        self._temporal_buffers(hi, self.info.rays_local)
        phase = density_phase(ft["k"])
        ft["k"] += 1
        self._check(self.foveate_density_phased_device(self._fd[0], self._fd[1], phase, hi.dmask))
        rendered, st = self.render_masked(hi.dmask, 1, None, self._o_rgb)
        rc, _ = self.fill_density_phased_device(hi.dmask, w, h, phase, self._o_rgb, self._rp_depth, self._rp_acc, None, count=False)
        self._check(rc)
        hist_rgb, hist_depth, hist_count, prev_pos, prev_rot, out = hi.inputs(self._pose)
        rejected = self.temporal_resolve_sparse_device(hi.dmask, phase, self._o_rgb, self._rp_depth, self._rp_acc, self._pose[0], self._pose[1], hist_rgb,
                                                       hist_depth, hist_count, prev_pos, prev_rot, out[0], out[1], out[2], hi.rgba, hi.mask,
                                                       alpha=ft["alpha"], depth_tol=ft["depth_tol"], clamp=ft["clamp"])
        hi.commit(self._pose)
        self._last_frame = (hi.rgba, w, h)
        self._rp_frame = None      # the depth between the rendered pixels is interpolated, not the volume's own
        return out[0].numpy(), hi.rgba.numpy(), hi.mask.numpy(), rejected, rendered, st

    # -- hybrid rendering: depth limits, the rasterised colour behind --------------------------------------
    def set_depth_limit(self, limit_zc=None):
        """Every ray of the frames rendered from now on stops at its entry of ``limit_zc`` (adanerf_set_depth_limit): [rays_local] fp32
        camera-space depths (the distance along the viewing axis; +inf or NaN: no limit for that ray).  A numpy array (uploaded into the
        renderer's own buffer), a device buffer (a DeviceArray, a pointer) or None (off).  A frame size that changes rays_local removes it."""
        if isinstance(limit_zc, np.ndarray):
            n = self.info.rays_local
            if limit_zc.size != n:
                raise ValueError("set_depth_limit: %d entries for %d local rays" % (limit_zc.size, n))
            self._buffers(("_dl_buf", (n,), np.float32))
            self.sync()      # frames in flight still read the buffer
            self._dl_buf.upload(limit_zc.reshape(-1).astype(np.float32, copy=False))
            limit_zc = self._dl_buf
        self._check(self.lib.adanerf_set_depth_limit(self.handle, _ptr(limit_zc)))
        self._dl_in_force = limit_zc

    def blend_behind(self, rgb, acc, behind_rgb, n: int, rgb_out=None, rgba8_out=None):
        """rgb + clamp(1 - acc, 0, 1) * behind_rgb over device [n,3] / [n] fp32 images into rgb_out ([n,3] fp32, may be rgb) and / or
        rgba8_out ([n] uchar4), on the context's stream (adanerf_blend_behind)"""
        self._check(self.lib.adanerf_blend_behind(self.handle, _ptr(rgb), _ptr(acc), _ptr(behind_rgb), int(n), _ptr(rgb_out), _ptr(rgba8_out)))

    sphere_zc = staticmethod(sphere_zc)

    def render_hybrid(self, limit_zc: np.ndarray, behind_rgb: np.ndarray):
        """One frame of the neural scene in front of rasterised geometry: ``limit_zc`` [rays_local] fp32 camera-space depths of the geometry
        (+inf where there is none), ``behind_rgb`` [rays_local,3] fp32 its colour.  Installs the limit, renders with the acc map attached,
        blends, and restores the limit and the aux outputs that were in force.  Returns (rgb [R,3] fp32, rgba8 [R,4] uint8, Stats of the
        render); the device copies stay in ``_o_rgb`` / ``_o_rgba`` as after render_numpy."""
        n = self.info.rays_local
        behind = np.ascontiguousarray(behind_rgb, dtype=np.float32).reshape(-1)
        if behind.size != 3 * n:
            raise ValueError("render_hybrid: %d colour values for %d local rays" % (behind.size, n))
        self._out_buffers()
        limit = np.ascontiguousarray(limit_zc, dtype=np.float32).reshape(-1)
        if limit.size != n:
            raise ValueError("render_hybrid: %d limits for %d local rays" % (limit.size, n))
        self._buffers(("_hy_acc", (n,), np.float32), ("_hy_behind", (n, 3), np.float32), ("_hy_limit", (n,), np.float32))
        was_limit, was_aux = self._dl_in_force, self._aux_in_force
        self.sync()      # frames in flight still read the buffers
        self._hy_behind.upload(behind)
        self._hy_limit.upload(limit)
        try:
            self.set_depth_limit(self._hy_limit)
            self.set_aux_outputs(was_aux[0], self._hy_acc)
            st = self.render(None, self._o_rgb, stats=True)
            self.blend_behind(self._o_rgb, self._hy_acc, self._hy_behind, n, self._o_rgb, self._o_rgba)
        finally:
            self.set_depth_limit(was_limit)
            self.set_aux_outputs(*was_aux)
        whole = n == self.info.width * self.info.height
        self._last_frame = (self._o_rgba, self.info.width, self.info.height) if whole else None
        self._rp_frame = None      # the blended frame's depth is not the volume's alone
        return self._o_rgb.numpy(), self._o_rgba.numpy(), st

    # -- anti-aliasing: sub-pixel offsets, accumulation ------------------------------------------------
    def set_pixel_offset(self, dx: float = 0.0, dy: float = 0.0):
        """The rays of the frames rendered from now on pass through (x + 0.5 + dx, y + 0.5 + dy) of their pixels (adanerf_set_pixel_offset):
        |dx|, |dy| <= 1, (0, 0) is the pixel centre.  Survives set_frame_size."""
        self._check(self.lib.adanerf_set_pixel_offset(self.handle, float(dx), float(dy)))

    @property
    def pixel_offset(self):
        """(dx, dy) in force"""
        out = (C.c_float * 2)()
        self._check(self.lib.adanerf_get_pixel_offset(self.handle, out))
        return float(out[0]), float(out[1])

    subpixel_grid = staticmethod(subpixel_grid)

    def accumulate_device(self, rgb, n_rays: int, sum_out, first: bool):
        """sum_out = rgb (first) or sum_out + rgb over device [n_rays,3] fp32 images, on the context's stream (adanerf_accumulate)"""
        self._check(self.lib.adanerf_accumulate(self.handle, _ptr(rgb), int(n_rays), _ptr(sum_out), 1 if first else 0))

    def resolve_mean_device(self, sum_in, n_rays: int, frames: int, rgba8_out=None, rgb_out=None):
        """sum_in / frames into rgb_out ([n_rays,3] fp32, may be sum_in) and / or rgba8_out ([n_rays] uchar4, the viewer's output contract),
        on the context's stream (adanerf_resolve_mean)"""
        self._check(self.lib.adanerf_resolve_mean(self.handle, _ptr(sum_in), int(n_rays), int(frames), _ptr(rgba8_out), _ptr(rgb_out)))

    def render_supersampled(self, s: int):
        """One anti-aliased frame: s*s renders at the offsets of subpixel_grid(s), accumulated and resolved on the device.  Returns
        (rgb_mean [R,3] fp32, rgba8 [R,4] uint8, Stats): the stage times are summed over the s*s renders, the sample counts are per rendered
        frame.  The device copies stay in ``_o_rgb`` / ``_o_rgba`` as after render_numpy (present() shows the resolved frame); the offset
        that was in force is restored."""
        grid = subpixel_grid(s)
        n = self.info.rays_local
        self._out_buffers()
        self._buffers(("_ss_sum", (n, 3), np.float32))
        was = self.pixel_offset
        total = Stats()
        try:
            for k, (dx, dy) in enumerate(grid):
                self.set_pixel_offset(dx, dy)
                st = self.render(None, self._o_rgb, stats=True)
                self.accumulate_device(self._o_rgb, n, self._ss_sum, first=k == 0)
                for name in ("ms_total", "ms_sample_mlp", "ms_compact", "ms_shade_mlp", "ms_composite", "total_samples", "batches", "shade_launches",
                             "sample_launches", "rays_refined"):
                    setattr(total, name, getattr(total, name) + getattr(st, name))
                for name in ("rays", "sampling_overflow", "guard_max_seen", "guard_violations", "guard_widened", "guard_pair_seen", "guard_audited",
                             "guard_audit_mismatch"):
                    setattr(total, name, getattr(st, name))
        finally:
            self.set_pixel_offset(*was)
        total.total_samples //= len(grid)
        total.rays_refined //= len(grid)
        self.resolve_mean_device(self._ss_sum, n, len(grid), self._o_rgba, self._o_rgb)
        whole = n == self.info.width * self.info.height
        self._last_frame = (self._o_rgba, self.info.width, self.info.height) if whole else None
        self._rp_frame = None      # the mean of several jittered frames has no single depth map to warp by
        self.last_stats = total
        return self._o_rgb.numpy(), self._o_rgba.numpy(), total

    # -- adaptive supersampling: the extra sub-pixel renders only at edges -------------------------------
    host_contrast_mask = staticmethod(host_contrast_mask)

    def contrast_mask(self, rgb, width: int, height: int, threshold: float, mask_out, count: bool = True):
        """adanerf_contrast_mask over device images: ``mask_out`` [height*width] uint8 gets 0 where a neighbour of the pixel differs from
        it by more than ``threshold`` in some channel's display value, 1 elsewhere.  Returns (code, n_flagged) instead of raising: tests
        look at both; ``count=False`` passes no counter (asynchronous, n_flagged is None)."""
        n = C.c_int32(-1)
        rc = self.lib.adanerf_contrast_mask(self.handle, _ptr(rgb), int(width), int(height), float(threshold), _ptr(mask_out), C.byref(n) if count else None)
        return rc, (int(n.value) if count else None)

    def accumulate_masked_device(self, rgb, mask, values: int, n_rays: int, sum_out, first: bool):
        """accumulate_device for the pixels ``mask`` selects (mask[p] < 32 and bit mask[p] of ``values``); every other pixel of sum_out
        keeps its bytes (adanerf_accumulate_masked)"""
        self._check(self.lib.adanerf_accumulate_masked(self.handle, _ptr(rgb), _ptr(mask), int(values) & 0xFFFFFFFF, int(n_rays), _ptr(sum_out), 1 if first else 0))

    def resolve_mean_masked_device(self, sum_in, mask, values: int, n_rays: int, frames: int, rgba8_out=None, rgb_out=None):
        """resolve_mean_device for the pixels ``mask`` selects; every other pixel of both outputs keeps its bytes
        (adanerf_resolve_mean_masked)"""
        self._check(self.lib.adanerf_resolve_mean_masked(self.handle, _ptr(sum_in), _ptr(mask), int(values) & 0xFFFFFFFF, int(n_rays), int(frames),
                                                         _ptr(rgba8_out), _ptr(rgb_out)))

    def render_supersampled_adaptive(self, s: int, threshold: float):
        """One anti-aliased frame at the cost of its edges: a render at the pixel centres (the centre frame), adanerf_contrast_mask on its
        fp32 colour, and -- if any pixel is flagged -- the s*s renders of subpixel_grid(s) for the flagged pixels alone
        (adanerf_render_masked), summed and averaged over the centre frame (adanerf_accumulate_masked / adanerf_resolve_mean_masked).  A
        flagged pixel carries the bytes render_supersampled(s) gives it, every other pixel the bytes of render_numpy().  s in
        2..SUPERSAMPLE_MAX, threshold in [0, 1].  Returns (rgb [R,3] fp32, rgba8 [R,4] uint8, mask [R] uint8 with 0 = refined, n_refined,
        Stats): the centre frame's record with the stage times summed over all passes.  The device copies stay in ``_o_rgb`` /
        ``_o_rgba``; the pixel offset that was in force is restored, and the aux / disparity maps in force hold the centre frame (they are
        switched off for the masked passes and put back)."""
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 2 <= s <= SUPERSAMPLE_MAX:
            raise ValueError("supersample: the adaptive form needs an integer S in 2..%d, got %r" % (SUPERSAMPLE_MAX, s))
        thr = float(threshold)
        if not (math.isfinite(thr) and 0.0 <= thr <= 1.0):
            raise ValueError("supersample contrast: the threshold must lie in [0, 1], got %r" % (threshold,))
        grid = subpixel_grid(s)
        n, w, h = self.info.rays_local, self.info.width, self.info.height
        if n != w * h:
            raise AdaNeRFError("render_supersampled_adaptive: whole frames only (shard_world must be 1): the contrast rule reads a pixel's neighbours")
        self._out_buffers()
        self._buffers(("_ss_sum", (n, 3), np.float32))
        self._buffers(("_sa_stage", (n, 3), np.float32), ("_sa_mask", (n,), np.uint8))
        was, was_aux, was_disp = self.pixel_offset, self._aux_in_force, self._disp_in_force
        try:
            self.set_pixel_offset(0.0, 0.0)
            total = self.render(self._o_rgba, self._o_rgb, stats=True)
            rc, flagged = self.contrast_mask(self._o_rgb, w, h, thr, self._sa_mask)
            self._check(rc)
            if flagged > 0:
                self.set_aux_outputs(None, None)      # the maps belong to the centre frame
                self.set_disp_output(None)
                for k, (dx, dy) in enumerate(grid):
                    self.set_pixel_offset(dx, dy)
                    _, st = self.render_masked(self._sa_mask, 1, None, self._sa_stage)
                    self.accumulate_masked_device(self._sa_stage, self._sa_mask, 1, n, self._ss_sum, first=k == 0)
                    for name in ("ms_total", "ms_sample_mlp", "ms_compact", "ms_shade_mlp", "ms_composite"):
                        setattr(total, name, getattr(total, name) + getattr(st, name))
                self.resolve_mean_masked_device(self._ss_sum, self._sa_mask, 1, n, len(grid), self._o_rgba, self._o_rgb)
        finally:
            self.set_pixel_offset(*was)
            if self._aux_in_force != was_aux:
                self.set_aux_outputs(*was_aux)
            if self._disp_in_force is not was_disp:
                self.set_disp_output(was_disp)
        self._last_frame = (self._o_rgba, w, h)
        self._rp_frame = None      # the refined pixels have no single depth to warp by
        self.last_stats = total
        return self._o_rgb.numpy(), self._o_rgba.numpy(), self._sa_mask.numpy(), flagged, total

    def render(self, rgba8_out=None, rgb_out=None, stats: bool = False) -> Optional[Stats]:
        """One frame into caller-owned device buffers ([rays_local] uchar4 / [rays_local,3] fp32).
        ``stats=True`` synchronises and returns the per-stage timing record."""
        st = Stats() if stats else None
        self._check(self.lib.adanerf_render(self.handle, _ptr(rgba8_out), _ptr(rgb_out), C.byref(st) if stats else None))
        if rgba8_out is not None:      # what present() shows: whole frames only (a shard's rows wait for adanerf_assemble_strips)
            whole = self.info.rays_local == self.info.width * self.info.height
            self._last_frame = (rgba8_out, self.info.width, self.info.height) if whole else None
        if stats:
            self.last_stats = st
        return st

    def render_masked(self, mask, values: int = 1, rgba8=None, rgb=None):
        """adanerf_render_masked: only the pixels p with mask[p] < 32 and bit mask[p] of ``values`` set are rendered, into the device
        images ``rgba8`` ([rays_local] uchar4) / ``rgb`` ([rays_local,3] fp32) -- at least one -- and into the aux maps in force; every
        other element keeps its bytes.  ``mask``: [rays_local] uint8 on the device (the masks of reproject / the temporal stages select
        directly: values=1 their holes, values=5 everything without a source pixel).  Returns (M, Stats of the M rays)."""
        st, m = Stats(), C.c_int32(0)
        self._check(self.lib.adanerf_render_masked(self.handle, _ptr(mask), int(values) & 0xFFFFFFFF, _ptr(rgba8), _ptr(rgb), C.byref(st), C.byref(m)))
        self.last_stats = st
        return int(m.value), st

    def set_aux_outputs(self, depth_map=None, acc_map=None):
        """Subsequent renders also fill [rays_local] fp32 depth_map (sum w z) / acc_map (sum w); None switches them off."""
        self._check(self.lib.adanerf_set_aux_outputs(self.handle, _ptr(depth_map), _ptr(acc_map)))
        self._aux_in_force = (depth_map, acc_map)      # render_hybrid puts them back

    def set_disp_output(self, disp_map=None):
        """Subsequent renders also fill [rays_local] fp32 disp_map = 1 / max(1e-10, depth_map / acc_map); None switches it off."""
        self._check(self.lib.adanerf_set_disp_output(self.handle, _ptr(disp_map)))
        self._disp_in_force = disp_map

    def gather_from(self, dst, src_renderer: "NeuralRenderer", src, nbytes: int):
        """Stream-ordered copy of ``nbytes`` from ``src`` (on ``src_renderer``'s device / stream) into ``dst`` on this
        renderer's device; this renderer's stream waits for it (single-process multi-GPU strip exchange)."""
        self._check(self.lib.adanerf_gather_to(self.handle, _ptr(dst), src_renderer.handle, _ptr(src), nbytes))

    def render_oracle(self, rgba8_out):
        """Sampling-network debug view of this rank's rays (the viewer's 'O' key): [rays_local] uchar4."""
        self._check(self.lib.adanerf_render_oracle(self.handle, _ptr(rgba8_out)))

    def copy_result_sampling_network(self, oracle, n_rays: int, rgba8_out):
        self._check(self.lib.adanerf_copy_result_sampling_network(self.handle, _ptr(oracle), n_rays, _ptr(rgba8_out)))

    def render_numpy(self):
        """Convenience for tests/tools: renders and returns (rgb fp32 [R,3], rgba8 [R,4], Stats).  The device copies stay in
        ``_o_rgb`` / ``_o_rgba`` until the next call (the evaluator scores the frame from there)."""
        n = self.info.rays_local
        self._out_buffers()
        if self._rp_on:
            self._reproject_buffers()
        st = self.render(self._o_rgba, self._o_rgb, stats=True)
        if self._rp_on:
            if self._pose is None:
                raise AdaNeRFError("reprojection needs the pose of the frame: call set_camera before render_numpy")
            self._rp_frame = (self._o_rgba, self._rp_depth, self._rp_acc, self._pose[0], self._pose[1], n)
            self.gather_from(self._rp_rgb, self, self._o_rgb, n * 12)      # the fp32 colour reproject_gather() taps, stream-ordered
        return self._o_rgb.numpy(), self._o_rgba.numpy(), st

    # -- the last frame at the pose of the moment --------------------------------------------------------
    def _reproject_buffers(self):
        """the renderer's own aux outputs and warp destinations, made on first use and again after a frame size that changes rays_local
        (the library drops the aux outputs then); installed as the context's aux outputs"""
        n = self.info.rays_local
        if self._buffers(("_rp_depth", (n,), np.float32), ("_rp_acc", (n,), np.float32), ("_rp_rgba", (n, 4), np.uint8), ("_rp_mask", (n,), np.uint8),
                         ("_rp_rgb", (n, 3), np.float32), ("_rp_wrgb", (n, 3), np.float32)):      # ... the frame's fp32 colour; the gathered one
            self._rp_frame = None
            self.set_aux_outputs(self._rp_depth, self._rp_acc)

    def enable_reprojection(self):
        """From now on render_numpy keeps what reproject() needs on the device: its RGBA8 frame, depth_map and acc_map in aux buffers of
        the renderer's own (they replace any set_aux_outputs of the caller's) and the pose of the last set_camera.  Whole frames of
        models without useNDC only (adanerf_reproject)."""
        if self.info.use_ndc or self.info.rays_local != self.info.width * self.info.height:
            raise AdaNeRFError("reprojection needs a whole frame of a model without useNDC")
        self._rp_on = True
        self._reproject_buffers()

    def reproject_device(self, src_rgba8, src_depth, src_acc, src_pos, src_rot, dst_pos, dst_rot, dst_rgba8, dst_depth=None, dst_mask=None,
                         acc_min: float = 0.5, hole_rgba8: int = 0xFF000000, fill: bool = True, holes: bool = True) -> Optional[int]:
        """adanerf_reproject on device images of the context's frame size: the frame (uchar4, depth_map, acc_map) rendered at
        (src_pos, src_rot) warped to (dst_pos, dst_rot) into dst_rgba8 and, if given, dst_depth (fp32) / dst_mask (uint8: 1 a source
        pixel, 2 filled from a neighbour, 0 hole_rgba8).  Returns the number of holes (synchronous); with holes=False nothing is read
        back and the outputs are complete after sync()."""
        fp = _pose_ptrs(src_pos, src_rot, dst_pos, dst_rot)
        n = C.c_int32(0)
        self._check(self.lib.adanerf_reproject(self.handle, _ptr(src_rgba8), _ptr(src_depth), _ptr(src_acc), fp[0], fp[1], fp[2], fp[3],
                                               float(acc_min), int(hole_rgba8) & 0xFFFFFFFF, REPROJECT_FILL if fill else 0, _ptr(dst_rgba8),
                                               _ptr(dst_depth), _ptr(dst_mask), C.byref(n) if holes else None))
        return int(n.value) if holes else None

    def reproject(self, dst_pos, dst_rot, fill: bool = True, acc_min: float = 0.5):
        """The last render_numpy frame (after enable_reprojection) warped to the pose (dst_pos, dst_rot): returns (rgba8 [R,4] uint8,
        mask [R] uint8, holes).  Holes come out opaque black.  The camera in force does not change."""
        if self._rp_frame is None or self._rp_frame[5] != self.info.rays_local:
            raise AdaNeRFError("reproject: no frame to warp -- enable_reprojection(), set_camera, then render_numpy")
        rgba, depth, acc, pos, rot, _ = self._rp_frame
        holes = self.reproject_device(rgba, depth, acc, pos, rot, dst_pos, dst_rot, self._rp_rgba, None, self._rp_mask, acc_min=acc_min, fill=fill)
        return self._rp_rgba.numpy(), self._rp_mask.numpy(), holes

    def reproject_rerender(self, dst_pos, dst_rot, rerender: str = "holes", fill: bool = True, acc_min: float = 0.5):
        """reproject(), then the pixels the warp could not source rendered at the destination pose into the warped colour:
        ``rerender="holes"`` the pixels nothing reached (mask 0), ``"unsourced"`` those filled from a neighbour as well (mask 0 and 2) --
        render_masked with values 1 / 5 over the warp's own mask.  The camera moves to (dst_pos, dst_rot) and stays there; the frame kept
        for warping (colour, depth_map, acc_map, its pose) is untouched: the aux maps belong to it and the next warp reads them, so they
        are switched off for the masked call and the warped depth is not re-rendered.  Returns (rgba8, mask, holes, rerendered).
        (A method of its own: reproject()'s signature is what its callers and tests know.)"""
        if rerender not in ("holes", "unsourced"):
            raise AdaNeRFError("reproject_rerender: rerender must be 'holes' or 'unsourced'")
        _, mask, holes = self.reproject(dst_pos, dst_rot, fill=fill, acc_min=acc_min)
        self.set_camera(dst_pos, dst_rot)
        self.set_aux_outputs(None, None)
        try:
            rerendered, _ = self.render_masked(self._rp_mask, RERENDER_VALUES[rerender], rgba8=self._rp_rgba)
        finally:
            self.set_aux_outputs(self._rp_depth, self._rp_acc)
        return self._rp_rgba.numpy(), mask, holes, rerendered

    # -- the same warp as a gather (adanerf_reproject_gather) ------------------------------------------------
    def reproject_gather_device(self, src_rgb, src_depth, src_acc, src_pos, src_rot, dst_pos, dst_rot, dst_rgb, dst_rgba8=None, dst_depth=None,
                                dst_mask=None, acc_min: float = 0.5, depth_tol: float = GATHER_DEPTH_TOL, iterations: int = GATHER_ITERATIONS,
                                hole_rgba8: int = 0xFF000000, guess: bool = True, holes: bool = True) -> Optional[int]:
        """adanerf_reproject_gather on device images of the context's frame size: the frame (fp32 rgb, depth_map, acc_map) rendered at
        (src_pos, src_rot) gathered at (dst_pos, dst_rot) into dst_rgb (fp32) and, if given, dst_rgba8 (uchar4) / dst_depth (fp32) /
        dst_mask (uint8: 1 a verified source surface, 2 an unverified one (guess), 0 hole).  Returns the number of holes (synchronous);
        with holes=False nothing is read back and the outputs are complete after sync()."""
        fp = _pose_ptrs(src_pos, src_rot, dst_pos, dst_rot)
        n = C.c_int32(0)
        self._check(self.lib.adanerf_reproject_gather(self.handle, _ptr(src_rgb), _ptr(src_depth), _ptr(src_acc), fp[0], fp[1], fp[2], fp[3],
                                                      float(acc_min), float(depth_tol), int(iterations), int(hole_rgba8) & 0xFFFFFFFF,
                                                      GATHER_GUESS if guess else 0, _ptr(dst_rgb), _ptr(dst_rgba8), _ptr(dst_depth),
                                                      _ptr(dst_mask), C.byref(n) if holes else None))
        return int(n.value) if holes else None

    def reproject_gather(self, dst_pos, dst_rot, iterations: int = GATHER_ITERATIONS, depth_tol: float = GATHER_DEPTH_TOL, guess: bool = True,
                         acc_min: float = 0.5):
        """The last render_numpy frame (after enable_reprojection) gathered at the pose (dst_pos, dst_rot): returns (rgb [R,3] float32,
        rgba8 [R,4] uint8, mask [R] uint8, holes).  Holes come out opaque black.  The camera in force does not change."""
        if self._rp_frame is None or self._rp_frame[5] != self.info.rays_local:
            raise AdaNeRFError("reproject_gather: no frame to warp -- enable_reprojection(), set_camera, then render_numpy")
        _, depth, acc, pos, rot, _ = self._rp_frame
        holes = self.reproject_gather_device(self._rp_rgb, depth, acc, pos, rot, dst_pos, dst_rot, self._rp_wrgb, self._rp_rgba, None, self._rp_mask,
                                             acc_min=acc_min, depth_tol=depth_tol, iterations=iterations, guess=guess)
        return self._rp_wrgb.numpy(), self._rp_rgba.numpy(), self._rp_mask.numpy(), holes

    def reproject_gather_rerender(self, dst_pos, dst_rot, rerender: str = "holes", iterations: int = GATHER_ITERATIONS,
                                  depth_tol: float = GATHER_DEPTH_TOL, guess: bool = True, acc_min: float = 0.5):
        """reproject_gather(), then the pixels the gather could not source rendered at the destination pose into the 8-bit colour, as
        reproject_rerender does for the splat: ``rerender="holes"`` the mask-0 pixels, ``"unsourced"`` the unverified ones (mask 2) as
        well.  The camera moves to (dst_pos, dst_rot) and stays there; the frame kept for warping is untouched.  Returns (rgba8, mask,
        holes, rerendered)."""
        if rerender not in ("holes", "unsourced"):
            raise AdaNeRFError("reproject_gather_rerender: rerender must be 'holes' or 'unsourced'")
        _, _, mask, holes = self.reproject_gather(dst_pos, dst_rot, iterations=iterations, depth_tol=depth_tol, guess=guess, acc_min=acc_min)
        self.set_camera(dst_pos, dst_rot)
        self.set_aux_outputs(None, None)
        try:
            rerendered, _ = self.render_masked(self._rp_mask, RERENDER_VALUES[rerender], rgba8=self._rp_rgba)
        finally:
            self.set_aux_outputs(self._rp_depth, self._rp_acc)
        return self._rp_rgba.numpy(), mask, holes, rerendered

    # -- two keyframes warped to a pose between them (adanerf_reproject_pair) ----------------------------------
    def reproject_pair_device(self, a_rgb, a_depth, a_acc, a_pos, a_rot, b_rgb, b_depth, b_acc, b_pos, b_rot, dst_pos, dst_rot, dst_rgb, dst_rgba8=None,
                              dst_depth=None, dst_mask=None, dst_source=None, weight_b: float = 0.5, acc_min: float = 0.5, depth_tol: float = 0.05,
                              hole_rgba8: int = 0xFF000000, fill: bool = True, holes: bool = True) -> Optional[int]:
        """adanerf_reproject_pair on device images of the context's frame size: the frames (fp32 rgb, depth_map, acc_map) rendered at
        (a_pos, a_rot) and (b_pos, b_rot) warped to (dst_pos, dst_rot) into dst_rgb (fp32) and, if given, dst_rgba8 (uchar4) / dst_depth
        (fp32) / dst_mask (uint8: 1 a source pixel, 2 filled from a neighbour, 0 hole) / dst_source (uint8: 1 A, 2 B, 3 both blended,
        0 none).  Returns the number of holes (synchronous); with holes=False nothing is read back and the outputs are complete after
        sync()."""
        fp = _pose_ptrs(a_pos, a_rot, b_pos, b_rot, dst_pos, dst_rot)
        n = C.c_int32(0)
        self._check(self.lib.adanerf_reproject_pair(self.handle, _ptr(a_rgb), _ptr(a_depth), _ptr(a_acc), fp[0], fp[1], _ptr(b_rgb), _ptr(b_depth),
                                                    _ptr(b_acc), fp[2], fp[3], fp[4], fp[5], float(weight_b), float(acc_min), float(depth_tol),
                                                    int(hole_rgba8) & 0xFFFFFFFF, REPROJECT_FILL if fill else 0, _ptr(dst_rgb), _ptr(dst_rgba8),
                                                    _ptr(dst_depth), _ptr(dst_mask), _ptr(dst_source), C.byref(n) if holes else None))
        return int(n.value) if holes else None

    def _interpolation_buffers(self):
        """the two source sets (fp32 colour, depth_map, acc_map) and the interpolated images, made on first use and again after a frame
        size that changes rays_local"""
        n = self.info.rays_local
        if self._buffers(("_ip_rgb0", (n, 3), np.float32), ("_ip_depth0", (n,), np.float32), ("_ip_acc0", (n,), np.float32),
                         ("_ip_rgb1", (n, 3), np.float32), ("_ip_depth1", (n,), np.float32), ("_ip_acc1", (n,), np.float32),
                         ("_ip_wrgb", (n, 3), np.float32), ("_ip_rgba", (n, 4), np.uint8), ("_ip_mask", (n,), np.uint8), ("_ip_source", (n,), np.uint8)):
            self._ip_keys = []

    def _ip_set(self, k: int):
        return (self._ip_rgb0, self._ip_depth0, self._ip_acc0) if k == 0 else (self._ip_rgb1, self._ip_depth1, self._ip_acc1)

    def enable_interpolation(self):
        """From now on render_keyframe() keeps the last two frames it rendered on the device -- fp32 colour, depth_map, acc_map and pose,
        in two sets that ping-pong -- and interpolate() warps both to a pose between them (adanerf_reproject_pair).  Whole frames of
        models without useNDC only.  The aux outputs point at the set being written during render_keyframe() and at what was in force
        before it afterwards."""
        if self.info.use_ndc or self.info.rays_local != self.info.width * self.info.height:
            raise AdaNeRFError("interpolation needs a whole frame of a model without useNDC")
        self._ip_on = True
        self._interpolation_buffers()

    def render_keyframe(self):
        """One render at the camera in force into the older of the two source sets (after enable_interpolation): it becomes the newer
        keyframe B, the one that was B becomes A.  Returns what render_numpy returns."""
        if not self._ip_on:
            raise AdaNeRFError("render_keyframe: call enable_interpolation() first")
        if self._pose is None:
            raise AdaNeRFError("interpolation needs the pose of the frame: call set_camera before render_keyframe")
        self._interpolation_buffers()
        self._out_buffers()
        k = 1 - self._ip_keys[-1][0] if self._ip_keys else 0
        rgb, depth, acc = self._ip_set(k)
        was = self._aux_in_force
        self.set_aux_outputs(depth, acc)
        try:
            st = self.render(self._o_rgba, rgb, stats=True)
        finally:
            self.set_aux_outputs(*was)
        self._ip_keys = self._ip_keys[-1:] + [(k, self._pose[0], self._pose[1])]
        return rgb.numpy(), self._o_rgba.numpy(), st

    def interpolate(self, dst_pos, dst_rot, weight_b: Optional[float] = None, fill: bool = True, acc_min: float = 0.5, depth_tol: float = 0.05):
        """The last two render_keyframe frames, A the older and B the newer, warped to the pose (dst_pos, dst_rot) between them: returns
        (rgb [R,3] float32, rgba8 [R,4] uint8, mask [R] uint8, source [R] uint8, holes).  ``weight_b``: the share of B where both see
        the same surface; None: pair_weight(dst_pos, A's position, B's).  Holes come out opaque black.  The camera in force does not
        change."""
        if len(self._ip_keys) < 2 or self._ip_mask is None or self._ip_mask.shape[0] != self.info.rays_local:
            raise AdaNeRFError("interpolate: needs two keyframes -- enable_interpolation(), then set_camera and render_keyframe twice")
        (ka, a_pos, a_rot), (kb, b_pos, b_rot) = self._ip_keys
        if weight_b is None:
            weight_b = pair_weight(dst_pos, a_pos, b_pos)
        holes = self.reproject_pair_device(*self._ip_set(ka), a_pos, a_rot, *self._ip_set(kb), b_pos, b_rot, dst_pos, dst_rot, self._ip_wrgb, self._ip_rgba,
                                           None, self._ip_mask, self._ip_source, weight_b=weight_b, acc_min=acc_min, depth_tol=depth_tol, fill=fill)
        return self._ip_wrgb.numpy(), self._ip_rgba.numpy(), self._ip_mask.numpy(), self._ip_source.numpy(), holes

    def interpolate_rerender(self, dst_pos, dst_rot, rerender: str = "holes", weight_b: Optional[float] = None, fill: bool = True, acc_min: float = 0.5,
                             depth_tol: float = 0.05):
        """interpolate(), then the pixels neither keyframe could source rendered at the destination pose into both colour images, as
        reproject_rerender does for the one-source warp: ``rerender="holes"`` the mask-0 pixels, ``"unsourced"`` the neighbour-filled
        ones (mask 2) as well.  The camera moves to (dst_pos, dst_rot) and stays there; the keyframes are untouched (the aux outputs are
        off for the masked call).  Returns (rgb, rgba8, mask, source, holes, rerendered)."""
        if rerender not in ("holes", "unsourced"):
            raise AdaNeRFError("interpolate_rerender: rerender must be 'holes' or 'unsourced'")
        _, _, mask, source, holes = self.interpolate(dst_pos, dst_rot, weight_b=weight_b, fill=fill, acc_min=acc_min, depth_tol=depth_tol)
        self.set_camera(dst_pos, dst_rot)
        was = self._aux_in_force
        self.set_aux_outputs(None, None)
        try:
            rerendered, _ = self.render_masked(self._ip_mask, RERENDER_VALUES[rerender], rgba8=self._ip_rgba, rgb=self._ip_wrgb)
        finally:
            self.set_aux_outputs(*was)
        return self._ip_wrgb.numpy(), self._ip_rgba.numpy(), mask, source, holes, rerendered

    # -- temporal anti-aliasing: one jittered render per frame, resolved against a history ------------------
    def temporal_resolve_device(self, cur_rgb, cur_depth, cur_acc, cur_pos, cur_rot, hist_rgb, hist_depth, hist_count, prev_pos, prev_rot,
                                out_rgb, out_depth=None, out_count=None, out_rgba8=None, out_mask=None, alpha: float = 0.1,
                                depth_tol: float = 0.02, acc_min: float = 0.5, clamp: bool = True, rejected: bool = True) -> Optional[int]:
        """adanerf_temporal_resolve on device images of the context's frame size: the frame (fp32 rgb, depth_map, acc_map) rendered at
        (cur_pos, cur_rot) blended with the history (rgb, depth, count: each may be None) the previous call wrote at (prev_pos, prev_rot)
        into out_rgb and, if given, out_depth / out_count (the next call's history), out_rgba8 and out_mask (uint8: 1 the history was
        used, 0 rejected).  Returns the number of rejected pixels (synchronous); with rejected=False nothing is read back and the outputs
        are complete after sync()."""
        fp = _pose_ptrs(cur_pos, cur_rot, prev_pos, prev_rot)
        n = C.c_int32(0)
        self._check(self.lib.adanerf_temporal_resolve(self.handle, _ptr(cur_rgb), _ptr(cur_depth), _ptr(cur_acc), fp[0], fp[1], _ptr(hist_rgb),
                                                      _ptr(hist_depth), _ptr(hist_count), fp[2], fp[3], float(alpha), float(depth_tol), float(acc_min),
                                                      TEMPORAL_CLAMP if clamp else 0, _ptr(out_rgb), _ptr(out_depth), _ptr(out_count),
                                                      _ptr(out_rgba8), _ptr(out_mask), C.byref(n) if rejected else None))
        return int(n.value) if rejected else None

    def _temporal_buffers(self, history: _History, n: int):
        """what a temporal stage renders into and resolves with: the frame's depth_map / acc_map (the aux buffers reproject() uses too),
        ``_o_rgb`` / ``_o_rgba``, and its history at n pixels -- each made on first use and again when its size changes"""
        self._reproject_buffers()
        self._out_buffers()
        history.ensure(n)

    def _render_next_offset(self, cycle):
        """One render into ``_o_rgb`` at the next sub-pixel offset of ``cycle`` (its "offsets" and the place "k" in them); the offset that
        was in force is restored.  Returns (dx, dy, Stats)."""
        dx, dy = cycle["offsets"][cycle["k"] % len(cycle["offsets"])]
        cycle["k"] += 1
        was = self.pixel_offset
        try:
            self.set_pixel_offset(dx, dy)
            st = self.render(None, self._o_rgb, stats=True)
        finally:
            self.set_pixel_offset(*was)
        return dx, dy, st

    def enable_temporal(self, alpha: float = 0.1, depth_tol: float = 0.02, clamp: bool = True, grid: int = 2):
        """Temporal anti-aliasing from now on through render_temporal(): every frame is rendered at the next offset of the grid x grid
        cycle of subpixel_grid and resolved against a history kept on the device (adanerf_temporal_resolve).  alpha in (0, 1]: the weight
        of the new frame once the history is older than 1 / alpha frames (until then it is a running mean); depth_tol: relative depth
        tolerance of the disocclusion test; clamp: the history is clamped to the new frame's 3 x 3 neighbourhood.  Whole frames of models
        without useNDC only.  The depth_map / acc_map aux outputs become the renderer's own (as with enable_reprojection)."""
        if self.info.use_ndc or self.info.rays_local != self.info.width * self.info.height:
            raise AdaNeRFError("temporal anti-aliasing needs a whole frame of a model without useNDC")
        alpha, depth_tol = _check_blend("enable_temporal", alpha, depth_tol)
        self._ta = dict(alpha=alpha, depth_tol=depth_tol, clamp=bool(clamp), offsets=subpixel_grid(grid), k=0)
        self._temporal_buffers(self._ta_history, self.info.rays_local)
        self._ta_history.reset()

    def reset_temporal(self):
        """Drops the history (a cut): the next render_temporal returns its frame as rendered.  The offset cycle goes on."""
        self._ta_history.reset()

    def render_temporal(self):
        """One frame at the camera of the last set_camera, rendered at the next sub-pixel offset of the cycle and resolved against the
        history, which it then replaces (two buffer sets ping-pong on the device).  Returns (rgb fp32 [R,3], rgba8 [R,4] uint8, mask [R]
        uint8, rejected, Stats): mask 1 where the history was used; rejected counts the others (every pixel on the first frame and after
        reset_temporal / set_frame_size).  While the pose is bit for bit the one of the call before, the history's depth is not tested
        (nothing is uncovered while the camera rests) and nothing is rejected.  The offset that was in force is restored; present()
        shows the resolved frame."""
        if self._ta is None:
            raise AdaNeRFError("render_temporal: call enable_temporal first")
        if self._pose is None:
            raise AdaNeRFError("render_temporal needs the pose of the frame: call set_camera first")
        ta, hi = self._ta, self._ta_history
        self._temporal_buffers(hi, self.info.rays_local)
        _, _, st = self._render_next_offset(ta)
        hist_rgb, hist_depth, hist_count, prev_pos, prev_rot, out = hi.inputs(self._pose)
        rejected = self.temporal_resolve_device(self._o_rgb, self._rp_depth, self._rp_acc, self._pose[0], self._pose[1], hist_rgb, hist_depth, hist_count,
                                                prev_pos, prev_rot, out[0], out[1], out[2], self._o_rgba, hi.mask, alpha=ta["alpha"],
                                                depth_tol=ta["depth_tol"], clamp=ta["clamp"])
        hi.commit(self._pose)
        self._last_frame = (self._o_rgba, self.info.width, self.info.height)
        self._rp_frame = None      # the aux maps now belong to a jittered frame whose colour was blended: nothing reproject() may warp
        return out[0].numpy(), self._o_rgba.numpy(), hi.mask.numpy(), rejected, st

    # -- temporal upsampling: one jittered render at w x h per frame, resolved into a history of s w x s h ----
    def temporal_upsample_device(self, scale: int, cur_rgb, cur_depth, cur_acc, cur_dx: float, cur_dy: float, cur_pos, cur_rot, hist_rgb, hist_depth,
                                 hist_count, prev_pos, prev_rot, out_rgb, out_depth=None, out_count=None, out_rgba8=None, out_mask=None,
                                 alpha: float = 0.1, depth_tol: float = 0.02, acc_min: float = 0.5, clamp: bool = True,
                                 rejected: bool = True) -> Optional[int]:
        """adanerf_temporal_upsample on device images: the frame (fp32 rgb, depth_map, acc_map) of the context's frame size w x h, rendered
        at (cur_pos, cur_rot) with the pixel offset (cur_dx, cur_dy), resolved into images of scale w x scale h: the history (rgb, depth,
        count: each may be None) the previous call wrote at (prev_pos, prev_rot), and out_rgb and, if given, out_depth / out_count (the
        next call's history), out_rgba8 and out_mask (uint8: 1 the history was used, 2 a placeholder replaced, 0 rejected).  Returns the
        number of rejected pixels (synchronous); with rejected=False nothing is read back and the outputs are complete after sync()."""
        fp = _pose_ptrs(cur_pos, cur_rot, prev_pos, prev_rot)
        n = C.c_int32(0)
        self._check(self.lib.adanerf_temporal_upsample(self.handle, int(scale), _ptr(cur_rgb), _ptr(cur_depth), _ptr(cur_acc), float(cur_dx), float(cur_dy),
                                                       fp[0], fp[1], _ptr(hist_rgb), _ptr(hist_depth), _ptr(hist_count), fp[2], fp[3], float(alpha),
                                                       float(depth_tol), float(acc_min), TEMPORAL_CLAMP if clamp else 0, _ptr(out_rgb), _ptr(out_depth),
                                                       _ptr(out_count), _ptr(out_rgba8), _ptr(out_mask), C.byref(n) if rejected else None))
        return int(n.value) if rejected else None

    def enable_temporal_upsample(self, scale: int = 2, alpha: float = 0.1, depth_tol: float = 0.02, clamp: bool = True):
        """Temporal upsampling from now on through render_upsampled(): every frame is rendered at the context's frame size w x h, at the
        next offset of the scale x scale cycle of subpixel_grid, and resolved into a history of scale w x scale h kept on the device
        (adanerf_temporal_upsample).  alpha, depth_tol, clamp: as enable_temporal's (the depth test is the neighbourhood one).  Whole
        frames of models without useNDC only.  The depth_map / acc_map aux outputs become the renderer's own."""
        if self.info.use_ndc or self.info.rays_local != self.info.width * self.info.height:
            raise AdaNeRFError("temporal upsampling needs a whole frame of a model without useNDC")
        if int(scale) != scale or not 1 <= int(scale) <= 4:
            raise ValueError("enable_temporal_upsample: scale must be 1, 2, 3 or 4, got %r" % (scale,))
        alpha, depth_tol = _check_blend("enable_temporal_upsample", alpha, depth_tol)
        self._tu = dict(scale=int(scale), alpha=alpha, depth_tol=depth_tol, clamp=bool(clamp), offsets=subpixel_grid(int(scale)), k=0)
        self._temporal_buffers(self._tu_history, self.info.rays_local * int(scale) ** 2)
        self._tu_history.reset()

    def reset_upsample(self):
        """Drops the history (a cut): the next render_upsampled shows every output pixel its nearest sample.  The offset cycle goes on."""
        self._tu_history.reset()

    def render_upsampled(self):
        """One frame at the camera of the last set_camera, rendered at w x h at the next sub-pixel offset of the cycle and resolved into
        the history of W x H = scale w x scale h, which it then replaces (two buffer sets ping-pong on the device).  Returns (rgb fp32
        [H*W,3], rgba8 [H*W,4] uint8, mask [H*W] uint8, rejected, Stats of the render): mask 1 where the history was used, 2 where it held
        only a placeholder; rejected counts mask 0 (every pixel on the first frame and after reset_upsample / set_frame_size).  While the
        pose is bit for bit the one of the call before, the history's depth is not tested (nothing is uncovered while the camera rests).
        The offset that was in force is restored; present() shows the upsampled frame."""
        if self._tu is None:
            raise AdaNeRFError("render_upsampled: call enable_temporal_upsample first")
        if self._pose is None:
            raise AdaNeRFError("render_upsampled needs the pose of the frame: call set_camera first")
        tu, hi = self._tu, self._tu_history
        self._temporal_buffers(hi, self.info.rays_local * tu["scale"] ** 2)
        dx, dy, st = self._render_next_offset(tu)
        hist_rgb, hist_depth, hist_count, prev_pos, prev_rot, out = hi.inputs(self._pose)
        rejected = self.temporal_upsample_device(tu["scale"], self._o_rgb, self._rp_depth, self._rp_acc, dx, dy, self._pose[0], self._pose[1], hist_rgb,
                                                 hist_depth, hist_count, prev_pos, prev_rot, out[0], out[1], out[2], hi.rgba, hi.mask,
                                                 alpha=tu["alpha"], depth_tol=tu["depth_tol"], clamp=tu["clamp"])
        hi.commit(self._pose)
        self._last_frame = (hi.rgba, self.info.width * tu["scale"], self.info.height * tu["scale"])
        self._rp_frame = None      # the aux maps now belong to a jittered frame: nothing reproject() may warp
        return out[0].numpy(), hi.rgba.numpy(), hi.mask.numpy(), rejected, st

    # -- the frame at the window's size ---------------------------------------------------------------
    def present_device(self, src_rgba8, src_w: int, src_h: int, dst_rgba8, dst_w: int, dst_h: int, flip_y: bool = False,
                       filter: Optional[str] = None):
        """The viewer's blit from its render buffer to the window (interoprenderbuffer.cpp:87) on device images: row-major uchar4
        [src_h*src_w] -> [dst_h*dst_w], on the context's stream (adanerf_present).  filter None: the reference's rule (linear if the
        destination is wider than the source, else nearest); "nearest" / "linear" force one; "area" is the exact area filter
        (ADANERF_PRESENT_AREA: a frame rendered larger than the window is averaged, not decimated; at most 8 to 1 per axis).
        flip_y: rows bottom-up (BMP order)."""
        if filter not in PRESENT_FILTERS:
            raise ValueError("present: filter must be None, 'nearest', 'linear' or 'area', got %r" % (filter,))
        self._check(self.lib.adanerf_present(self.handle, _ptr(src_rgba8), int(src_w), int(src_h), _ptr(dst_rgba8), int(dst_w), int(dst_h),
                                             (PRESENT_FLIP_Y if flip_y else 0) | PRESENT_FILTERS[filter]))

    def present(self, window_w: Optional[int] = None, window_h: Optional[int] = None, flip_y: bool = False,
                filter: Optional[str] = None) -> np.ndarray:
        """The last rendered frame (render_numpy, or a render() with an rgba8 buffer) at the window's size: uint8
        [window_h, window_w, 4].  Default size: settings.window_width / window_height.  Whole frames only (shard_world 1)."""
        if self._last_frame is None:
            raise AdaNeRFError("present: no whole frame has been rendered into an rgba8 buffer yet (a shard's strips: assemble them, then present_device)")
        src, w, h = self._last_frame
        ww, wh = int(window_w or self.settings.window_width), int(window_h or self.settings.window_height)
        dst = DeviceArray(self, (wh, ww, 4), np.uint8)
        try:
            self.present_device(src, w, h, dst, ww, wh, flip_y=flip_y, filter=filter)
            return dst.numpy()
        finally:
            dst.free()

    # -- image metrics -----------------------------------------------------------------------------
    def flip_device(self, test_rgb, ref_rgb, width: int, height: int, pixels_per_degree: Optional[float] = None, error_map=None,
                    mean: bool = True) -> Optional[float]:
        """FLIP of two device images ([height*width, 3] fp32 sRGB, the layout of render()'s rgb_out) as the reference's evaluation
        computes it (src/evaluate.py:120-145 over src/util/flip_loss.py).  error_map: optional device [height*width] fp32.  Returns the
        mean error (synchronous); with mean=False nothing is read back and the map is complete after sync().  pixels_per_degree None:
        the reference's 67.02."""
        m = C.c_float(0)
        self._check(self.lib.adanerf_flip(self.handle, _ptr(test_rgb), _ptr(ref_rgb), width, height,
                                          0.0 if pixels_per_degree is None else float(pixels_per_degree), _ptr(error_map),
                                          C.byref(m) if mean else None))
        return float(m.value) if mean else None

    def flip(self, test_rgb, ref_rgb, width: Optional[int] = None, height: Optional[int] = None, pixels_per_degree: Optional[float] = None,
             return_map: bool = False):
        """FLIP of two host images: numpy [h, w, 3], or [h*w, 3] with width / height given (default: this renderer's frame).  Returns
        the mean, or (mean, map [h, w] fp32) with return_map."""
        t, r = np.asarray(test_rgb, dtype=np.float32), np.asarray(ref_rgb, dtype=np.float32)
        if t.shape != r.shape:
            raise ValueError("flip: images differ in shape: %s and %s" % (t.shape, r.shape))
        if t.ndim == 3 and t.shape[2] == 3:
            h, w = t.shape[:2]
            if (width not in (None, w)) or (height not in (None, h)):
                raise ValueError("flip: %dx%d images, width / height say %sx%s" % (w, h, width, height))
        elif t.ndim == 2 and t.shape[1] == 3:
            w, h = width or self.settings.width, height or self.settings.height
            if w * h != t.shape[0]:
                raise ValueError("flip: %d pixels are not %d x %d" % (t.shape[0], w, h))
        else:
            raise ValueError("flip: expected [h, w, 3] or [h*w, 3], got %s" % (t.shape,))
        bufs = [DeviceArray(self, (h * w, 3), np.float32).upload(t.reshape(-1, 3)), DeviceArray(self, (h * w, 3), np.float32).upload(r.reshape(-1, 3))]
        if return_map:
            bufs.append(DeviceArray(self, (h * w,), np.float32))
        try:
            mean = self.flip_device(bufs[0], bufs[1], w, h, pixels_per_degree, bufs[2] if return_map else None)
            return (mean, bufs[2].numpy().reshape(h, w)) if return_map else mean
        finally:
            for b in bufs:
                b.free()

    def sync(self):
        self._check(self.lib.adanerf_sync(self.handle))

    def set_stream(self, hip_stream: Optional[int]):
        """Enqueue on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)."""
        self._check(self.lib.adanerf_set_stream(self.handle, hip_stream))

    def set_profiling(self, enabled: bool):
        self._check(self.lib.adanerf_set_profiling(self.handle, 1 if enabled else 0))

    def collect_stats(self):
        """(Stats summed over the frames rendered since the last collect, number of frames)."""
        st = Stats()
        n = C.c_int32(0)
        self._check(self.lib.adanerf_collect_stats(self.handle, C.byref(st), C.byref(n)))
        return st, n.value

    def assemble_strips(self, gathered, image_out):
        self._check(self.lib.adanerf_assemble_strips(self.handle, _ptr(gathered), _ptr(image_out)))

    def buffer(self, which: int, dtype, shape) -> np.ndarray:
        """Copies an internal buffer of the last rendered batch to the host."""
        p = C.c_void_p()
        nb = C.c_size_t()
        self._check(self.lib.adanerf_get_buffer(self.handle, which, C.byref(p), C.byref(nb)))
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= nb.value, (out.nbytes, nb.value)
        if out.nbytes:
            self._check(self.lib.adanerf_memcpy_d2h(self.handle, out.ctypes.data, p.value, out.nbytes))
        return out

    # -- stage-level entry points --------------------------------------------------------------------
    def ray_features(self, first_ray: int, n_rays: int, features_out=None, rays_out=None):
        self._check(self.lib.adanerf_ray_features(self.handle, first_ray, n_rays, _ptr(features_out), _ptr(rays_out)))

    def sample_mlp(self, first_ray: int, n_rays: int, oracle_out=None, rays_out=None):
        self._check(self.lib.adanerf_sample_mlp(self.handle, first_ray, n_rays, _ptr(oracle_out), _ptr(rays_out)))

    def compact(self, oracle, n_rays: int, n_max: int, thr: float, ray_offsets, ray_counts, sample_key, sample_w, total):
        self._check(self.lib.adanerf_compact(self.handle, _ptr(oracle), n_rays, n_max, thr, _ptr(ray_offsets),
                                             _ptr(ray_counts), _ptr(sample_key), _ptr(sample_w), _ptr(total)))

    def compact_depth_limit(self, oracle, n_rays: int, n_max: int, thr: float, rays, limit_zc, pos, rot_c2w, ray_offsets, ray_counts, sample_key,
                            sample_w, total) -> int:
        """adanerf_compact_depth_limit: the selection at (n_max, thr), the depth trim of ray r to limit_zc[r] under the pose (pos, rot_c2w)
        with the ray records ``rays`` [n_rays,8], then the compaction.  Returns the library's code instead of raising: tests look at both."""
        p, r = _pose_ptrs(pos, rot_c2w)
        return self.lib.adanerf_compact_depth_limit(self.handle, _ptr(oracle), n_rays, n_max, thr, _ptr(rays), _ptr(limit_zc), p, r, _ptr(ray_offsets), _ptr(ray_counts), _ptr(sample_key), _ptr(sample_w), _ptr(total))

    def compact_cap(self, oracle, n_rays: int, n_max: int, thr: float, cap_total: int, ray_offsets, ray_counts, sample_key, sample_w, total, tstar,
                    n_map=None, thr_map=None, rays=None, limit_zc=None, pos=None, rot_c2w=None) -> int:
        """adanerf_compact_cap: the selection at (n_max, thr), the budget trim (n_map / thr_map) and the depth trim (rays, limit_zc, pos,
        rot_c2w) where given, the sample cap at C = cap_total, then the compaction; ``tstar`` [1] fp32 on the device gets t* (-inf: nothing
        trimmed).  Returns the library's code instead of raising: tests look at both."""
        p, r = _pose_ptrs(pos, rot_c2w)
        return self.lib.adanerf_compact_cap(self.handle, _ptr(oracle), n_rays, n_max, thr, _ptr(n_map), _ptr(thr_map), _ptr(rays), _ptr(limit_zc), p, r, int(cap_total),
                                            _ptr(ray_offsets), _ptr(ray_counts), _ptr(sample_key), _ptr(sample_w), _ptr(total), _ptr(tstar))

    def compact_budget(self, oracle, n_rays: int, n_max: int, thr: float, n_map, thr_map, ray_offsets, ray_counts, sample_key, sample_w, total):
        self._check(self.lib.adanerf_compact_budget(self.handle, _ptr(oracle), n_rays, n_max, thr, _ptr(n_map), _ptr(thr_map), _ptr(ray_offsets),
                                                    _ptr(ray_counts), _ptr(sample_key), _ptr(sample_w), _ptr(total)))

    def compact_guarded(self, oracle_approx, oracle_exact, n_rays: int, n_max: int, thr: float, eps: float, ray_offsets, ray_counts,
                        sample_key, sample_w, total, refined, eps_pair: float = 0.0, audit_period: int = 0, audit_phase: int = 0, monitor=None,
                        audit_fill_cap: int = 0, audit_cycle: int = 0):
        """monitor: optional device uint32[5] the caller zeroed (largest error bits, rows beyond a bound, largest pair error bits,
        audit mismatches, audited rows)."""
        self._check(self.lib.adanerf_compact_guarded(self.handle, _ptr(oracle_approx), _ptr(oracle_exact), n_rays, n_max, thr, eps, eps_pair,
                                                     audit_period, audit_phase, audit_fill_cap, audit_cycle, _ptr(ray_offsets), _ptr(ray_counts), _ptr(sample_key),
                                                     _ptr(sample_w), _ptr(total), _ptr(refined), _ptr(monitor)))

    def refresh_info(self) -> "Info":
        """Re-reads adanerf_info (guard_eps moves when the band is calibrated or widened after a violation)."""
        self._check(self.lib.adanerf_get_info(self.handle, C.byref(self.info)))
        return self.info

    def calibrate_guard(self, n_poses: int = 8, seed: int = 1, install: bool = False, pair: bool = False):
        """Largest |plain-fp16 - split-precision| raw output over n_poses x 4096 calibration rays (pair=True: also the largest
        error of a (kept - candidate) difference, as a tuple); install=True makes ADANERF_GUARD_CALIB_MARGIN x those the context's
        bounds and writes the model's calibration record."""
        d, dp = C.c_float(0), C.c_float(0)
        self._check(self.lib.adanerf_calibrate_guard(self.handle, n_poses, seed, 1 if install else 0, C.byref(d), C.byref(dp)))
        if install:
            self._check(self.lib.adanerf_get_info(self.handle, C.byref(self.info)))
        return (float(d.value), float(dp.value)) if pair else float(d.value)

    def guard_calibration_file(self) -> str:
        """Path of the calibration record of this context's (model, N, threshold)."""
        n = self.lib.adanerf_guard_calibration_file(self.handle, None, 0)
        if n < 0:
            self._check(n)
        buf = C.create_string_buffer(n)
        self.lib.adanerf_guard_calibration_file(self.handle, buf, n)
        return buf.value.decode()

    def probe_mfma(self, operands: str = "relu", f16: bool = False, target_ms: float = 100.0):
        """(TFLOP/s, MHz) this device sustains on register-only 16-bit MFMA loops with "zero" / "constant" / "random" / "relu" operands
        (include/adanerf_hip.h adanerf_probe_mfma)."""
        tf, mhz = C.c_float(0), C.c_float(0)
        self._check(self.lib.adanerf_probe_mfma(self.handle, {"zero": 0, "constant": 1, "random": 2, "relu": 3}[operands], 1 if f16 else 0,
                                                target_ms, C.byref(tf), C.byref(mhz)))
        return float(tf.value), float(mhz.value)

    def shade_features(self, rays, sample_key, n_samples: int, features_out):
        self._check(self.lib.adanerf_shade_features(self.handle, _ptr(rays), _ptr(sample_key), n_samples, _ptr(features_out)))

    def shade_mlp(self, rays, sample_key, total, max_samples: int, raw_out, precision: int = -1):
        self._check(self.lib.adanerf_shade_mlp(self.handle, _ptr(rays), _ptr(sample_key), _ptr(total), max_samples,
                                               precision, _ptr(raw_out)))

    def shade_mlp_z(self, rays, sample_key, sample_z, total, max_samples: int, raw_out, precision: int = -1):
        self._check(self.lib.adanerf_shade_mlp_z(self.handle, _ptr(rays), _ptr(sample_key), _ptr(sample_z), _ptr(total),
                                                 max_samples, precision, _ptr(raw_out)))

    def sample_pdf(self, oracle, n_rays: int, n: int, ray_offsets, ray_counts, sample_key, sample_w, sample_z, total):
        self._check(self.lib.adanerf_sample_pdf(self.handle, _ptr(oracle), n_rays, n, _ptr(ray_offsets), _ptr(ray_counts),
                                                _ptr(sample_key), _ptr(sample_w), _ptr(sample_z), _ptr(total)))

    # vanilla NeRF (SAMPLER_COARSE_FINE): uniform coarse samples, the coarse network, the fine sampler
    def sample_uniform(self, first_ray: int, n_rays: int, rays, ray_offsets, ray_counts, sample_key, total):
        self._check(self.lib.adanerf_sample_uniform(self.handle, first_ray, n_rays, _ptr(rays), _ptr(ray_offsets), _ptr(ray_counts),
                                                    _ptr(sample_key), _ptr(total)))

    def shade_mlp_coarse(self, rays, sample_key, total, max_samples: int, raw_out, precision: int = -1):
        self._check(self.lib.adanerf_shade_mlp_coarse(self.handle, _ptr(rays), _ptr(sample_key), _ptr(total), max_samples, precision, _ptr(raw_out)))

    def sample_from_coarse(self, raw_coarse, rays, n_rays: int, ray_offsets, ray_counts, sample_key, sample_z, total):
        self._check(self.lib.adanerf_sample_from_coarse(self.handle, _ptr(raw_coarse), _ptr(rays), n_rays, _ptr(ray_offsets), _ptr(ray_counts),
                                                        _ptr(sample_key), _ptr(sample_z), _ptr(total)))

    def composite_classic(self, raw, sample_z, rays, n_rays: int, n: int, rgb_out=None, rgba8_out=None):
        self._check(self.lib.adanerf_composite_classic(self.handle, _ptr(raw), _ptr(sample_z), _ptr(rays), n_rays, n,
                                                       _ptr(rgb_out), _ptr(rgba8_out)))

    def composite(self, raw, sample_w, ray_offsets, ray_counts, n_rays: int, rgb_out=None, rgba8_out=None):
        self._check(self.lib.adanerf_composite(self.handle, _ptr(raw), _ptr(sample_w), _ptr(ray_offsets), _ptr(ray_counts),
                                               n_rays, _ptr(rgb_out), _ptr(rgba8_out)))

    def composite_aux(self, raw, sample_w, ray_offsets, ray_counts, sample_key, n_rays: int, rgb_out=None, rgba8_out=None, depth_out=None,
                      acc_out=None):
        """composite that also writes depth_map / acc_map [n_rays] fp32; sample_key None: dense contexts only (bin = sample index & 127)"""
        self._check(self.lib.adanerf_composite_aux(self.handle, _ptr(raw), _ptr(sample_w), _ptr(ray_offsets), _ptr(ray_counts), _ptr(sample_key),
                                                   n_rays, _ptr(rgb_out), _ptr(rgba8_out), _ptr(depth_out), _ptr(acc_out)))

    def composite_classic_aux(self, raw, sample_z, rays, n_rays: int, n: int, rgb_out=None, rgba8_out=None, depth_out=None, acc_out=None):
        self._check(self.lib.adanerf_composite_classic_aux(self.handle, _ptr(raw), _ptr(sample_z), _ptr(rays), n_rays, n,
                                                           _ptr(rgb_out), _ptr(rgba8_out), _ptr(depth_out), _ptr(acc_out)))

    def disp_map(self, depth, acc, n: int, disp_out):
        """disp_out[i] = 1 / max(1e-10, depth[i] / acc[i]) over n fp32 values (NaN stays NaN)"""
        self._check(self.lib.adanerf_disp_map(self.handle, _ptr(depth), _ptr(acc), n, _ptr(disp_out)))


# The names tests and tools read the histories by (``_ta_sets``, ``_ta_hist``, ``_tu_rgba``, ``_ft_dmask``, ...): read-only views of the
# members of the history objects.
for _mode, _members in (("ta", ("sets", "hist", "mask")), ("tu", ("sets", "hist", "mask", "rgba")), ("ft", ("sets", "hist", "mask", "rgba", "dmask"))):
    for _member in _members:
        setattr(NeuralRenderer, "_%s_%s" % (_mode, _member),
                property(lambda self, _h="_%s_history" % _mode, _m=_member: getattr(getattr(self, _h), _m)))
