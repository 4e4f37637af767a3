// The depth-tangent renderer (ns_tangent.h) on an f16 field: the 16-bit kernel of ns_nerf_mlp_ob16.hip with TWO primal tiles of 16
// samples per wave and their tangents as register tiles 2 and 3 (groups of 128 samples), the register footprint of the forward's
// four-tile generic kernel (492 VGPRs + AGPRs at W = 256, 278 at W = 128).  The primal tiles' rgb / disp / depth / acc are the bits
// of ns_nerf_forward_ob16's one-kernel renderer; the tangents are carried in fp16, through v_sin as the forward's encoding.
#include "ns_tangent.h"

namespace {

template <class M, int NKB>
__global__ void __launch_bounds__(nstan::kWaves * 64)
nerf_tan16_kernel(nstan::TanArgs a) {
  nstan::tangent_body<M, NKB>(a);
}

}  // namespace

// called by ns_render_rays_fused_tangent (ns_render.cpp) for an f16 handle
int ns_nerf_forward_ob16_tangent(const ns_weights* net, const float* o_dev, const float* d_dev, const float* viewdirs_dev,
                                 int64_t R, int N, const ns_composite_args* comp, float* d_rgb, float* d_disp, float* d_depth,
                                 float* d_acc, hipStream_t stream) {
  using M = nsmlp::Mma16F16;
  nstan::TanArgs a{};
  const int rc = nstan::fill_tan_args<M>(a, net, o_dev, d_dev, viewdirs_dev, R, N, comp, d_rgb, d_disp, d_depth, d_acc);
  if (rc != NS_OK) return rc;
  // (only f16 is instantiated: bf16 fields are refused)
  if (net->dtype == NS_DTYPE_F16)
    return net->width == 256 ? nstan::launch_tan<M>(nerf_tan16_kernel<M, 8>, a, stream)
                             : nstan::launch_tan<M>(nerf_tan16_kernel<M, 4>, a, stream);
  ns::set_error("ns_render_rays_fused_tangent: an f16 handle is required here (dtype %d)", net->dtype);
  return NS_E_UNSUPPORTED;
}
