// Internal layout of the opaque ns_weights handle (host side) and the entry points the library's files call in one another.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct ns_weights {
  int kind;       // 0 = NeRF, 1 = DepthNet
  int dtype;      // NS_DTYPE_*
  int width;      // hidden width the kernels run (128 or 256): every layer is zero-padded to it at pack time
  int depth;      // NeRF: D;  DepthNet: number of trunk layers (the skip branches are folded into trunk layer 0)
  int skip;       // NeRF: first skip index or -1 (legacy view of skip_mask)
  uint32_t skip_mask;   // NeRF: bit i set <=> i in skips, i.e. layer i + 1 sees cat[x, h] (run_nerf_helpers.py:117-118)
  int use_viewdirs;     // NeRF: 1 = alpha / feature / views / rgb head (:120-131), 0 = output_linear (:132-133)
  int out_ch;           // NeRF: channels of raw (4 with view directions; output_ch of output_linear otherwise)
  int layout;     // weight stream order: 0 = k-major slabs (consume<>), 16 = 16x16x32 output-sub-block-major (layer_ob16<>)
  void* stream_dev;      // weight stream, n_slabs * 16 KiB, consumed cyclically by every workgroup
  uint32_t n_slabs;
  float* bias_dev;       // all biases in LDS image order, fp32
  int bias_floats;
  // 16-bit production field (8 x 256, skips = [4], view directions; bf16 / f16) only, else NULL: the SIGMA-FIRST stream of the
  // render kernel (ns_nerf_mlp_ob16.hip) -- the same n_slabs, the same chunks with the same contents, the tail re-ordered into
  // three slab-aligned statements: the view layer's sigma sub-block | its eight colour sub-blocks | the rgb head -- and the
  // bias image in that order (bias_floats as well)
  void* stream2_dev;
  float* bias2_dev;
  int kbskip_ok;         // 1: every 16-bit weight of the sigma-first stream is finite (the K-block-skipping render kernel may run)
  int unit_ordered;      // 1: the caller packed the hidden units by firing rate (ns_weights_set_unit_ordered): dead K-blocks are
                         // mostly a suffix of a layer's output, which the dead-suffix render kernel is built for
};

enum { NS_KIND_NERF = 0, NS_KIND_DEPTHNET = 1 };

// Per-ray outputs of a radiance-field pass that composites in its own epilogue (internal: ns_render.cpp -> the 16-bit MLP
// kernel).  mean_dev != NULL: the kernel also PLACES the samples (sample_points_around_mean "uniform") from the DepthNet
// depth; otherwise depths come from the z array given to the forward call.
struct ns_composite_args {
  const float* mean_dev;   // [R] or NULL
  float std_;
  int white_bkgd;
  float* rgb_dev; int64_t rgb_stride;
  float* disp_dev; int64_t disp_stride;
  float* weights_dev;      // [R,N] or NULL
  float* z_out_dev;        // [R,N] or NULL
  float* pts_out_dev;      // [R,N,3] or NULL
  const float* sigma_last_dev;   // NULL, or [R,4] raw of every ray's LAST sample from the guard pass: its sigma (element 3)
                                 // replaces the kernel's own for that sample (ns_render_args::nerf_guard)
  // the selective guard (ns_render_args::guard_threshold > 0): records of the rays whose own |sigma_last| < fix_thr (laid out in
  // ns_guard.h), counted in *fix_count_dev (zeroed by the caller)
  float fix_thr;
  uint32_t* fix_count_dev;
  float* fix_rec_dev;
  // the max-weight sample of every ray (ns_hier_args::max_z_dev ..): all three or none (NULL: not produced)
  float* max_z_dev;        // [R]
  float* max_w_dev;        // [R]
  float* max_rgb_dev;      // [R,3]
  // the per-ray expected depth sum_i w_i z_i and opacity sum_i w_i (ns_render_args::depth_dev / acc_dev), each NULL when not wanted
  float* depth_dev;        // [R]
  float* acc_dev;          // [R]
};
bool ns_nerf_can_composite(const ns_weights* net, int N);

// The layout-16 kernels behind the public forwards and the one-call renderers (arguments validated by the callers).
// ns_nerf_forward / ns_nerf_forward_embedded on a layout-16 handle; comp: composite (and place) in the kernel (ns_nerf_mlp_ob16.hip)
int ns_nerf_forward_ob16(const ns_weights* net, const float* pts_dev, const float* o_dev, const float* d_dev,
                         const float* z_dev, const float* viewdirs_dev, const float* x90_dev, int64_t S, int N,
                         float* raw_dev, hipStream_t stream, const ns_composite_args* comp);
// ... on an NS_DTYPE_F16X3 handle; count_dev: the selective guard's fix-up (ns_nerf_mlp_x3.hip)
int ns_nerf_forward_x3(const ns_weights* net, const float* pts_dev, const float* o_dev, const float* d_dev,
                       const float* z_dev, const float* viewdirs_dev, const float* x90_dev, int64_t S, int N,
                       float* raw_dev, hipStream_t stream, const uint32_t* count_dev, const ns_composite_args* comp);
// ns_render_rays_fused_tangent on an f16x3 / an f16 field (ns_nerf_mlp_x3_tan.hip, ns_nerf_mlp_ob16_tan.hip)
int ns_nerf_forward_x3_tangent(const ns_weights* net, const float* o_dev, const float* d_dev, const float* viewdirs_dev, int64_t R,
                               int N, const ns_composite_args* comp, float* d_rgb, float* d_disp, float* d_depth, float* d_acc,
                               hipStream_t stream);
int ns_nerf_forward_ob16_tangent(const ns_weights* net, const float* o_dev, const float* d_dev, const float* viewdirs_dev,
                                 int64_t R, int N, const ns_composite_args* comp, float* d_rgb, float* d_disp, float* d_depth,
                                 float* d_acc, hipStream_t stream);
// ns_depthnet_forward on a layout-16 handle (ns_depthnet_ob16.hip)
int ns_depthnet_forward_ob16(const ns_weights* net, const float* o_dev, const float* d_dev, int64_t R, float near_,
                             float far_, float sphere_radius, float* z_dev, hipStream_t stream);
