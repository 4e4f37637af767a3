// The depth-tangent renderer (ns_tangent.h) on an f16x3 field: the split-fp16 kernel of ns_nerf_mlp_x3.hip with ONE primal tile of
// 16 samples per wave and its tangent as the second register tile (groups of 64 samples; 432 VGPRs + AGPRs at W = 256, 249 at
// W = 128).  The primal tile's rgb / disp / depth / acc are the bits of ns_nerf_forward_x3's one-kernel renderer.
// nerf_mlp_x3_tan1_kernel is the one-sample-per-ray form (NS_MODE_DEPTH_ONLY: a group is 64 rays, each finished by the lanes that
// hold it): its rgb is the bits of ns_nerf_forward_x3 at N = 1 composited by ns_raw2outputs.
#include "ns_tangent.h"

namespace {

using M = nsmlp::Mma16F16x3;

template <int NKB>
__global__ void __launch_bounds__(nstan::kWaves * 64)
nerf_mlp_x3_tan_kernel(nstan::TanArgs a) {
  nstan::tangent_body<M, NKB>(a);
}

template <int NKB>
__global__ void __launch_bounds__(nstan::kWaves * 64)
nerf_mlp_x3_tan1_kernel(nstan::TanArgs a) {
  nstan::tangent_body<M, NKB, true>(a);
}

}  // namespace

// called by ns_render_rays_fused_tangent (ns_render.cpp) for an f16x3 handle; N == 1 is the one-sample render of
// NS_MODE_DEPTH_ONLY (uniform placement has N >= 2)
int ns_nerf_forward_x3_tangent(const ns_weights* net, const float* o_dev, const float* d_dev, const float* viewdirs_dev, int64_t R,
                               int N, const ns_composite_args* comp, float* d_rgb, float* d_disp, float* d_depth, float* d_acc,
                               hipStream_t stream) {
  nstan::TanArgs a{};
  const int rc = nstan::fill_tan_args<M>(a, net, o_dev, d_dev, viewdirs_dev, R, N, comp, d_rgb, d_disp, d_depth, d_acc);
  if (rc != NS_OK) return rc;
  if (N == 1)
    return net->width == 256 ? nstan::launch_tan<M>(nerf_mlp_x3_tan1_kernel<8>, a, stream)
                             : nstan::launch_tan<M>(nerf_mlp_x3_tan1_kernel<4>, a, stream);
  return net->width == 256 ? nstan::launch_tan<M>(nerf_mlp_x3_tan_kernel<8>, a, stream)
                           : nstan::launch_tan<M>(nerf_mlp_x3_tan_kernel<4>, a, stream);
}
