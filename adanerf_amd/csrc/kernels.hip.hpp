// gfx950 (CDNA4, wave64) kernels of the AdaNeRF per-frame hot path.  Device code only; the C ABI
// in adanerf_hip.hip launches these (the fp32-MFMA ones through launch_f32.hip).  The plain structs the host fills are in params.hpp.
// Every kernel is compiled in exactly one unit: A* and N8 in adanerf_hip.hip, through this file; the others in stages.hip.  Stage map:
//   A1+A2+A3  sample_mlp_kernel      ray gen -> sphere exit -> oracle PE -> 8-layer sampling MLP (fp32 MFMA)
//   A4        select_kernel / scan_blocks_kernel / expand_kernel   top-N + threshold, deterministic compaction
//   A4b       trim_rows_kernel / trim_rows_wave_kernel / foveate_kernel   per-ray budgets: the selection trimmed to (n_r, thr_r), the maps of a gaze
//   A4c       depth_limit_kernel     per-ray depth limits: the selection trimmed to the samples in front of a rasterised surface
//   A4d       cap_hist_kernel / cap_search_kernel / cap_fill_kernel   a bound on the batch's samples: the threshold t* that meets it, by an exact radix selection
//   A5+A6     shade_mlp16x2_kernel / shade_mlp32_kernel   fused PE + 8x256 shading MLP (bf16/f16/f32 MFMA)
//   A7        composite_kernel       sigmoid + alpha * oracle weight, front-to-back
//   N8        mask_bits_kernel / mask_scatter_kernel   a byte mask as bit words for refine_list_kernel; the pixels of a listed batch to their places (masked rendering)
// stages.hip (k_flip, k_present, k_reproject, k_reproject_gather, k_reproject_pair, k_accumulate, k_temporal, k_upsample, k_blend, k_density, k_sparse_temporal, k_contrast;
// k_pose_core: the arithmetic N4, N13, N14, N6, N7 and N12 share):
//   N1        flip_kernel / flip_mean_kernel   FLIP error map and mean of an image pair (the evaluator's second metric)
//   N3        present_kernel / present_area_kernel   the frame at the window's size (the viewer's blit: linear / nearest, y flip; exact area filter)
//   N4        reproject_clear_kernel / reproject_splat_kernel / reproject_resolve_kernel   a rendered frame warped to another pose by its depth
//   N13       gather_surface_kernel / gather_warp_kernel   the same warp as a gather: each destination pixel iterates along its ray to the source surface
//   N14       reproject_pair_splat_kernel / reproject_pair_resolve_kernel   two rendered frames warped to a pose between them: N4's splat per source, one resolve over both z-buffers
//   N5        accumulate_kernel / resolve_mean_kernel   sum and mean of several sub-pixel frames (supersampling in time)
//   N6        temporal_resolve_kernel   a history image carried to the pose of the moment, clamped and blended with the new frame (temporal anti-aliasing)
//   N7        upsample_depth_kernel / upsample_resolve_kernel   a frame rendered at w x h resolved into a history of s w x s h (temporal upsampling)
//   N9        blend_behind_kernel   the rasterised colour behind a depth-limited frame, through the transmittance that is left (hybrid rendering)
//   N10       density_mask_kernel / density_fill_kernel   the render mask of a gaze and rings of strides; the pixels between the rendered ones, bilinear (foveated ray density)
//   N12       sparse_resolve_kernel   the temporal resolve of a foveated frame: rendered pixels refresh the history, reconstructed ones keep it (phased lattice)
//   N11       contrast_mask_kernel / accumulate_masked_kernel / resolve_mean_masked_kernel   the pixels on an edge of a rendered frame; sum and mean of the sub-pixel renders of those alone (adaptive supersampling)
// plus, in adanerf_hip.hip, explicit-feature debug kernels (ray_features_kernel, shade_features_kernel) that materialise
// what the reference launchers wrote to memory, for parity tests only.
// The code lives in one header per stage; this file includes those of adanerf_hip.hip.
#pragma once
#include "k_common.hip.hpp"
#include "k_mlp_f32.hip.hpp"
#include "k_compact.hip.hpp"
#include "k_select_pair.hip.hpp"
#include "k_mlp16.hip.hpp"
#include "k_sampling16.hip.hpp"
#include "k_donerf.hip.hpp"
#include "k_coarse_fine.hip.hpp"
#include "k_composite.hip.hpp"
#include "k_budget.hip.hpp"
#include "k_mask.hip.hpp"
#include "k_depth_limit.hip.hpp"
#include "k_cap.hip.hpp"
