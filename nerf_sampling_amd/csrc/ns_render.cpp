// The DepthNet branch of render_rays_test (nerf_utils.py:836-865) as one call: a fixed chain of
// kernel launches on the caller's stream, intermediates in a caller-provided workspace.
#include "ns_common.h"
#include "ns_guard.h"
#include "ns_weights.h"

namespace {

inline int64_t align256(int64_t x) { return (x + 255) & ~static_cast<int64_t>(255); }

// Hands out 256-byte-aligned slices of a workspace in order and keeps the running total.  Each renderer's layout below is
// written once: its *_workspace_bytes function runs it on a null base and returns the total, the renderer runs it on the
// caller's workspace.
struct Carve {
  char* base = nullptr;
  int64_t total = 0;
  float* take(int64_t bytes) {
    float* p = base ? reinterpret_cast<float*>(base + total) : nullptr;
    total += align256(bytes);
    return p;
  }
};

struct RaySlices { float *o, *d, *view; };
RaySlices take_rays(Carve& ws, int64_t R) { return {ws.take(R * 12), ws.take(R * 12), ws.take(R * 12)}; }

struct ChainLayout { RaySlices rays; float *mean, *z_last, *raw_last, *z, *raw; };
ChainLayout chain_layout(Carve& ws, int64_t R, int N) {
  ChainLayout l;
  l.rays = take_rays(ws, R);
  l.mean = ws.take(R * 4);
  l.z_last = ws.take(R * 4);          // the guard pass (ns_render_args::nerf_guard): depth and raw of every ray's last sample
  l.raw_last = ws.take(R * 16);
  l.z = ws.take(R * N * 4); l.raw = ws.take(R * N * 16);
  return l;
}

struct FusedLayout { RaySlices rays; float *mean, *z_last, *raw_last; uint32_t* fix_count; float* fix_rec; RaySlices fix_rays; };
// rec_floats: the selective guard's record (ns_guard.h) -- nsfix::kLongFloats on rays of several chunks
// (ns_render_args::guard_long_selective); every other call keeps nsfix::kFloats, the layout and the size it has had
constexpr int64_t kFixCountBytes = 256;   // the selective guard's counter, a slice of its own
FusedLayout fused_layout(Carve& ws, int64_t R, int rec_floats) {
  FusedLayout l;
  l.rays = take_rays(ws, R);
  l.mean = ws.take(R * 4);
  l.z_last = ws.take(R * 4);          // the every-ray guard's depth and raw of the last sample; the selective guard's z and raw
  l.raw_last = ws.take(R * 16);       // of the flagged rays' last samples
  l.fix_count = reinterpret_cast<uint32_t*>(ws.take(kFixCountBytes));   // the selective guard: counter, records, compacted rays
  l.fix_rec = ws.take(R * rec_floats * 4);
  l.fix_rays = take_rays(ws, R);
  return l;
}

struct TangentLayout { RaySlices rays; float* mean; };
TangentLayout tangent_layout(Carve& ws, int64_t R) {
  TangentLayout l;
  l.rays = take_rays(ws, R);
  l.mean = ws.take(R * 4);            // the DepthNet depth, when the caller supplies none
  return l;
}

// max_slice: the call produces the max-weight sample -- one more slice at the end, the fine weights of the chain's argmax when
// the caller takes none (every slice before it stays where it is)
struct HierLayout { RaySlices rays; float *z_c, *raw_c, *w_c, *z_f, *raw_f, *w_f; };
HierLayout hier_layout(Carve& ws, int64_t R, int Nc, int Nt, bool max_slice) {
  HierLayout l;
  l.rays = take_rays(ws, R);
  l.z_c = ws.take(R * Nc * 4); l.raw_c = ws.take(R * Nc * 16); l.w_c = ws.take(R * Nc * 4);
  l.z_f = ws.take(R * Nt * 4); l.raw_f = ws.take(R * Nt * 16);
  l.w_f = max_slice ? ws.take(R * Nt * 4) : nullptr;
  return l;
}

struct Rays { int64_t R = 0; const float *o = nullptr, *d = nullptr, *view = nullptr; };   // R = 0: nothing to render

// The ray source of the three renderers: explicit rays (o_dev != NULL, R of them) or rows [row0, row1) of the camera image,
// generated into the o / d / viewdirs slices of the renderer's layout.  carve_layout(ws, R) lays the workspace out for R rays
// and returns those slices.
template <class Args, class CarveLayout>
int resolve_rays(const Args* a, CarveLayout carve_layout, Rays* r, void* stream) {
  *r = Rays{};
  if (a->o_dev == nullptr ? (a->row1 == a->row0 || a->W == 0) : a->R == 0) return NS_OK;  // nothing to render
  NS_REQUIRE(a->workspace_dev && a->rgb_dev && a->disp_dev, "workspace, rgb and disp are required");
  NS_REQUIRE(a->o_dev || (a->row0 >= 0 && a->row1 <= a->H && a->row0 <= a->row1 && a->W > 0), "bad camera rows");
  NS_REQUIRE(!a->o_dev || (a->d_dev && a->viewdirs_dev), "explicit rays need o, d and viewdirs");
  NS_REQUIRE((reinterpret_cast<uintptr_t>(a->workspace_dev) & 255) == 0, "workspace must be 256-byte aligned");
  const int64_t R = a->o_dev ? a->R : static_cast<int64_t>(a->row1 - a->row0) * a->W;
  Carve ws{static_cast<char*>(a->workspace_dev)};
  const RaySlices s = carve_layout(ws, R);
  if (a->o_dev) { *r = Rays{R, a->o_dev, a->d_dev, a->viewdirs_dev}; return NS_OK; }
  const int rc = ns_get_rays(a->H, a->W, a->fx, a->fy, a->cx, a->cy, a->c2w, a->row0, a->row1, a->near_, a->far_, s.o, s.d,
                             s.view, nullptr, stream);
  if (rc == NS_OK) *r = Rays{R, s.o, s.d, s.view};
  return rc;
}

// The caller's per-ray outputs, strides resolved (0 = packed: 3 / 1).
struct Outputs { float* rgb; int64_t rgb_stride; float* disp; int64_t disp_stride; float* weights; float* depth; float* acc; };
template <class Args>
Outputs outputs(const Args* a) {
  return {a->rgb_dev, a->rgb_stride ? a->rgb_stride : 3, a->disp_dev, a->disp_stride ? a->disp_stride : 1, a->weights_dev,
          a->depth_dev, a->acc_dev};
}

// raw [R,N,4] composited into the caller's rgb / disp (/ weights, depth, acc)
int composite(const Outputs& out, const float* raw, const float* z, const float* d, int64_t R, int N, int white_bkgd,
              void* stream) {
  return ns_raw2outputs_strided(raw, z, d, nullptr, R, N, white_bkgd, out.rgb, out.rgb_stride, out.disp, out.disp_stride,
                                out.acc, out.depth, nullptr, out.weights, stream);
}
// the per-ray outputs of a pass that composites in the MLP kernel's epilogue
void set_outputs(ns_composite_args& c, const Outputs& out) {
  c.rgb_dev = out.rgb; c.rgb_stride = out.rgb_stride; c.disp_dev = out.disp; c.disp_stride = out.disp_stride;
  c.weights_dev = out.weights; c.depth_dev = out.depth; c.acc_dev = out.acc;
}

// an optional event (NULL = none) recorded on the stream
int record(void* ev, void* stream) { return ev ? ns_event_record(ev, stream) : NS_OK; }

// ns::prod_tiles_hint() for the MLP launch in its scope (see ns_common.h): 4 when the call has per-sample outputs, whose host
// copies will run beside the next MLP kernel; reset on the way out
struct ProdTilesHint {
  explicit ProdTilesHint(const ns_render_args* a) { ns::prod_tiles_hint() = (a->z_dev || a->weights_dev || a->pts_dev) ? 4 : 0; }
  ~ProdTilesHint() { ns::prod_tiles_hint() = 0; }
};

// The guard pass: the last sample of every ray through a second, fp32-grade (F16X3) handle of the same network; its raw
// lands in raw_last [R,4].  (nerf_utils.py:836-865 composites that sample with dist = 1e10, sampling_trainer.py:176-180.)
// guard_check runs before a renderer launches anything.
int guard_check(const ns_render_args* a) {
  const ns_weights* gnet = a->nerf_guard;
  if (!(gnet->kind == NS_KIND_NERF && gnet->out_ch == 4 && gnet->use_viewdirs && gnet->width == a->nerf->width &&
        gnet->depth == a->nerf->depth && gnet->skip_mask == a->nerf->skip_mask)) {
    ns::set_error("nerf_guard must be another packing of the same network (a NeRF with view directions, same D / W / skips)");
    return NS_E_INVALID;
  }
  if (a->mode != NS_MODE_UNIFORM || a->N < 2) {
    ns::set_error("nerf_guard: the guard pass is defined for uniform placement with n_samples >= 2");
    return NS_E_UNSUPPORTED;
  }
  return NS_OK;
}
int guard_pass(const ns_render_args* a, const Rays& r, const float* mean, float* z_last, float* raw_last, void* stream) {
  const int rc = ns_place_last_sample(mean, r.R, a->N, a->std_, z_last, stream);
  if (rc != NS_OK) return rc;
  return ns_nerf_forward(a->nerf_guard, nullptr, r.o, r.d, z_last, r.view, r.R, 1, raw_last, stream);
}

}  // namespace

extern "C" {

int64_t ns_render_workspace_bytes(int64_t R, int N) {
  if (R < 0 || N < 1) return 0;
  Carve ws;
  chain_layout(ws, R, N);
  return ws.total;
}

int ns_render_rays_depthnet(const ns_render_args* a, void* stream) {
  NS_REQUIRE(a, "null args");
  NS_REQUIRE(a->depthnet && a->nerf, "both networks are required");
  NS_REQUIRE(a->nerf->kind == NS_KIND_NERF && a->nerf->out_ch == 4 && a->nerf->use_viewdirs,
             "the one-call path composites raw [R,N,4] of a network with view directions");
  const int N = a->mode == NS_MODE_DEPTH_ONLY ? 1 : a->N;
  NS_REQUIRE(N >= 1, "bad sample count");
  int rc = a->nerf_guard ? guard_check(a) : NS_OK;
  if (rc != NS_OK) return rc;
  ChainLayout l;
  Rays r;
  rc = resolve_rays(a, [&](Carve& ws, int64_t R) { l = chain_layout(ws, R, N); return l.rays; }, &r, stream);
  if (rc != NS_OK || r.R == 0) return rc;
  float* z = a->z_dev ? a->z_dev : l.z;
  rc = ns_depthnet_forward(a->depthnet, r.o, r.d, r.R, a->near_, a->far_, a->sphere_radius, l.mean, stream);
  if (rc != NS_OK) return rc;
  rc = ns_place_samples(a->mode, r.o, r.d, l.mean, a->noise_dev, r.R, N, a->std_, a->pts_dev, z, stream);
  if (rc != NS_OK) return rc;
  if ((rc = record(a->ev_mlp_begin, stream)) != NS_OK) return rc;
  {
    ProdTilesHint hint(a);
    rc = ns_nerf_forward(a->nerf, nullptr, r.o, r.d, z, r.view, r.R, N, l.raw, stream);
  }
  if (rc != NS_OK) return rc;
  if ((rc = record(a->ev_mlp_end, stream)) != NS_OK) return rc;
  if (a->nerf_guard) {
    rc = guard_pass(a, r, l.mean, l.z_last, l.raw_last, stream);
    if (rc != NS_OK) return rc;
    rc = ns_patch_sigma_last(l.raw, l.raw_last, r.R, N, stream);
    if (rc != NS_OK) return rc;
  }
  return composite(outputs(a), l.raw, z, r.d, r.R, N, a->white_bkgd, stream);
}

// ---- the same branch as ONE kernel per ray tile: rays -> DepthNet -> [placement + radiance-field
// MLP + compositing in one persistent kernel].  Per-sample data (z, pts, raw, weights) never reaches HBM unless asked for.
int ns_render_fused_supported(const ns_weights* nerf, int mode, int N) {
  return mode == NS_MODE_UNIFORM && ns_nerf_can_composite(nerf, N) ? 1 : 0;
}

int64_t ns_render_fused_workspace_bytes(int64_t R) {
  if (R < 0) return 0;
  Carve ws;
  fused_layout(ws, R, nsfix::kFloats);
  return ws.total;
}

int64_t ns_render_fused_guard_long_workspace_bytes(int64_t R) {
  if (R < 0) return 0;
  Carve ws;
  fused_layout(ws, R, nsfix::kLongFloats);
  return ws.total;
}

int ns_render_rays_fused(const ns_render_args* a, void* stream) {
  NS_REQUIRE(a, "null args");
  NS_REQUIRE(a->depthnet && a->nerf, "both networks are required");
  if (!ns_render_fused_supported(a->nerf, a->mode, a->N)) {
    ns::set_error("ns_render_rays_fused: uniform placement, a bf16, f16 or f16x3 NeRF handle with view directions and n_samples "
                  "a power of two in [2, 64] or a multiple of 64 up to 512 are required (mode %d, N %d); use ns_render_rays_depthnet",
                  a->mode, a->N);
    return NS_E_UNSUPPORTED;
  }
  NS_REQUIRE(!a->noise_dev, "uniform placement takes no noise");
  int rc = a->nerf_guard ? guard_check(a) : NS_OK;
  if (rc != NS_OK) return rc;
  // (the fix-up launches the split-operand MLP kernel with a device-side count: another packing of the guard handle, e.g. fp32,
  // takes the every-ray pass through the generic dispatch.  An f16x3 field is fp32-grade itself: its guard is the every-ray one)
  // Rays of several chunks take the selective form only when the caller opts in (guard_long_selective): an unflagged ray keeps
  // its 16-bit sigma, and callers of N > 64 have had the every-ray guard's bits on every ray.
  const bool long_rays = a->N > 64;
  const bool selective = a->nerf_guard && a->guard_threshold > 0.0f && (!long_rays || a->guard_long_selective == 1) &&
                         a->nerf_guard->dtype == NS_DTYPE_F16X3 && a->nerf_guard->layout == 16 && a->nerf->dtype != NS_DTYPE_F16X3;
  const int rec_floats = selective && long_rays ? nsfix::kLongFloats : nsfix::kFloats;
  FusedLayout l;
  Rays r;
  rc = resolve_rays(a, [&](Carve& ws, int64_t R) { l = fused_layout(ws, R, rec_floats); return l.rays; }, &r, stream);
  if (rc != NS_OK || r.R == 0) return rc;
  rc = ns_depthnet_forward(a->depthnet, r.o, r.d, r.R, a->near_, a->far_, a->sphere_radius, l.mean, stream);
  if (rc != NS_OK) return rc;
  const Outputs out = outputs(a);
  ns_composite_args c{};
  c.mean_dev = l.mean; c.std_ = a->std_; c.white_bkgd = a->white_bkgd;
  set_outputs(c, out);
  c.z_out_dev = a->z_dev; c.pts_out_dev = a->pts_dev;
  if (selective) {         // the kernel flags the rays itself; their last samples are re-evaluated after it
    c.fix_thr = a->guard_threshold;
    c.fix_count_dev = l.fix_count;
    c.fix_rec_dev = l.fix_rec;
    NS_HIP(hipMemsetAsync(l.fix_count, 0, kFixCountBytes, ns::as_stream(stream)));
  } else if (a->nerf_guard) {     // (before the event pair: the pair times the fused kernel alone)
    rc = guard_pass(a, r, l.mean, l.z_last, l.raw_last, stream);
    if (rc != NS_OK) return rc;
    c.sigma_last_dev = l.raw_last;
  }
  if ((rc = record(a->ev_mlp_begin, stream)) != NS_OK) return rc;
  {
    ProdTilesHint hint(a);
    rc = ns_nerf_forward_ob16(a->nerf, nullptr, r.o, r.d, nullptr, r.view, nullptr, r.R * a->N, a->N, nullptr,
                              ns::as_stream(stream), &c);
  }
  if (rc != NS_OK) return rc;
  if ((rc = record(a->ev_mlp_end, stream)) != NS_OK) return rc;
  if (!selective) return NS_OK;
  const RaySlices& fr = l.fix_rays;
  rc = ns_fix_gather(l.fix_rec, rec_floats, l.fix_count, r.R, r.o, r.d, r.view, fr.o, fr.d, fr.view, l.z_last, stream);
  if (rc != NS_OK) return rc;
  rc = ns_nerf_forward_x3(a->nerf_guard, nullptr, fr.o, fr.d, l.z_last, fr.view, nullptr, r.R, 1, l.raw_last,
                          ns::as_stream(stream), l.fix_count, nullptr);
  if (rc != NS_OK) return rc;
  rc = ns_fix_last_sample(l.fix_rec, rec_floats, l.fix_count, r.R, l.raw_last, a->N, a->white_bkgd, out.rgb, out.rgb_stride,
                          out.disp, out.disp_stride, out.weights, out.depth, out.acc, stream);
  if (rc != NS_OK || !a->guard_count_dev) return rc;
  NS_HIP(hipMemcpyAsync(a->guard_count_dev, l.fix_count, sizeof(uint32_t), hipMemcpyDeviceToDevice, ns::as_stream(stream)));
  return NS_OK;
}

// ---- the one-kernel renderer with forward-mode tangents in the DepthNet depth (ns_tangent.h, instantiated by
// ns_nerf_mlp_x3_tan.hip for an f16x3 field and by ns_nerf_mlp_ob16_tan.hip for an f16 one): the rays' Jacobians
// d {rgb, disp, depth, acc} / d mean beside the forward's outputs
int ns_render_tangent_supported(const ns_weights* nerf, int mode, int N) {
  if (!nerf) return 0;
  // one sample per ray at the DepthNet depth: the f16x3 instance only (training wants the fp32-grade Jacobian), at any N
  if (mode == NS_MODE_DEPTH_ONLY)
    return nerf->kind == NS_KIND_NERF && nerf->layout == 16 && nerf->dtype == NS_DTYPE_F16X3 && nerf->use_viewdirs &&
           nerf->out_ch == 4 ? 1 : 0;
  return (nerf->dtype == NS_DTYPE_F16X3 || nerf->dtype == NS_DTYPE_F16) && ns_render_fused_supported(nerf, mode, N) ? 1 : 0;
}

int64_t ns_render_tangent_workspace_bytes(int64_t R) {
  if (R < 0) return 0;
  Carve ws;
  tangent_layout(ws, R);
  return ws.total;
}

int ns_render_rays_fused_tangent(const ns_render_args* a, const ns_tangent_args* t, void* stream) {
  NS_REQUIRE(a && t, "null args");
  NS_REQUIRE(a->nerf, "the NeRF handle is required");
  NS_REQUIRE(t->mean_dev || a->depthnet, "a DepthNet handle or the caller's mean is required");
  const int N = a->mode == NS_MODE_DEPTH_ONLY ? 1 : a->N;     // one sample per ray: N and std_ are ignored (ns_place_samples)
  if (!ns_render_tangent_supported(a->nerf, a->mode, a->N)) {
    ns::set_error("ns_render_rays_fused_tangent: uniform placement with an f16x3 or f16 NeRF handle with view directions and n_samples "
                  "a power of two in [2, 64] or a multiple of 64 up to 512, or depth_only placement with an f16x3 one, are "
                  "required (mode %d, N %d, dtype %d)", a->mode, a->N, a->nerf->dtype);
    return NS_E_UNSUPPORTED;
  }
  NS_REQUIRE(!a->noise_dev, "uniform and depth_only placement take no noise");
  if (a->nerf_guard || a->z_dev || a->weights_dev || a->pts_dev) {
    ns::set_error("ns_render_rays_fused_tangent: no guard pass and no per-sample outputs (z, weights, pts)");
    return NS_E_UNSUPPORTED;
  }
  TangentLayout l;
  Rays r;
  int rc = resolve_rays(a, [&](Carve& ws, int64_t R) { l = tangent_layout(ws, R); return l.rays; }, &r, stream);
  if (rc != NS_OK || r.R == 0) return rc;
  const float* mean = t->mean_dev;
  if (!mean) {
    rc = ns_depthnet_forward(a->depthnet, r.o, r.d, r.R, a->near_, a->far_, a->sphere_radius, l.mean, stream);
    if (rc != NS_OK) return rc;
    mean = l.mean;
  }
  ns_composite_args c{};
  c.mean_dev = mean; c.std_ = a->std_; c.white_bkgd = a->white_bkgd;
  set_outputs(c, outputs(a));
  if ((rc = record(a->ev_mlp_begin, stream)) != NS_OK) return rc;
  if (a->nerf->dtype == NS_DTYPE_F16X3)
    rc = ns_nerf_forward_x3_tangent(a->nerf, r.o, r.d, r.view, r.R, N, &c, t->d_rgb_dev, t->d_disp_dev, t->d_depth_dev,
                                    t->d_acc_dev, ns::as_stream(stream));
  else
    rc = ns_nerf_forward_ob16_tangent(a->nerf, r.o, r.d, r.view, r.R, a->N, &c, t->d_rgb_dev, t->d_disp_dev, t->d_depth_dev,
                                      t->d_acc_dev, ns::as_stream(stream));
  if (rc != NS_OK) return rc;
  return record(a->ev_mlp_end, stream);
}

int64_t ns_hier_workspace_bytes(int64_t R, int Nc, int Nf) {
  if (R < 0 || Nc < 3 || Nf < 0) return 0;
  Carve ws;
  hier_layout(ws, R, Nc, Nc + Nf, false);
  return ws.total;
}

int64_t ns_hier_max_workspace_bytes(int64_t R, int Nc, int Nf) {
  if (R < 0 || Nc < 3 || Nf < 0) return 0;
  Carve ws;
  hier_layout(ws, R, Nc, Nc + Nf, true);
  return ws.total;
}

int ns_render_rays_hierarchical(const ns_hier_args* a, void* stream) {
  NS_REQUIRE(a && a->coarse, "null args / coarse network");
  NS_REQUIRE(a->coarse->out_ch == 4 && a->coarse->use_viewdirs && (!a->fine || (a->fine->out_ch == 4 && a->fine->use_viewdirs)),
             "the one-call path composites raw [R,N,4] of networks with view directions");
  NS_REQUIRE(a->Nc >= 3 && a->Nf >= 0, "needs at least 3 coarse samples");
  const bool max_sample = a->max_z_dev || a->max_w_dev || a->max_rgb_dev;
  NS_REQUIRE(!max_sample || (a->max_z_dev && a->max_w_dev && a->max_rgb_dev), "max_z, max_w and max_rgb go together");
  NS_REQUIRE(!max_sample || a->Nf > 0, "the max-weight sample is one of the fine pass: needs n_importance > 0");
  const int Nc = a->Nc, Nt = a->Nc + a->Nf;
  HierLayout l;
  Rays r;
  int rc = resolve_rays(a, [&](Carve& ws, int64_t R) { l = hier_layout(ws, R, Nc, Nt, max_sample); return l.rays; }, &r, stream);
  if (rc != NS_OK || r.R == 0) return rc;
  const int64_t R = r.R;
  const Outputs out = outputs(a);
  // coarse pass (Trainer.py:579-649); its rgb/disp are not part of the 8-tuple and are not produced
  rc = ns_coarse_z_scalar(a->near_, a->far_, R, Nc, a->lindisp, a->t_rand_dev, l.z_c, stream);
  if (rc != NS_OK) return rc;
  if ((rc = record(a->ev_coarse_begin, stream)) != NS_OK) return rc;
  // A bf16 / f16 / f16x3 field composites in its own epilogue (nsepi::CompFields::comp == 1: depths from the z array): raw [R,N,4] -- 16 bytes
  // per sample written and read back, 2.6 GB per 800 x 800 frame at 64 + 192 samples -- then never exists.  The coarse
  // pass only yields its weights (its colour goes to a scratch corner of the unused raw_c block).
  const bool chain = ns::debug_flags().hier_chain != 0;
  const bool fuse_c = !chain && a->Nf > 0 && ns_nerf_can_composite(a->coarse, Nc);
  if (fuse_c) {
    ns_composite_args c{};
    c.white_bkgd = a->white_bkgd;
    c.rgb_dev = l.raw_c; c.rgb_stride = 4; c.disp_dev = l.raw_c + 3; c.disp_stride = 4;
    c.weights_dev = l.w_c;
    rc = ns_nerf_forward_ob16(a->coarse, nullptr, r.o, r.d, l.z_c, r.view, nullptr, R * Nc, Nc, nullptr, ns::as_stream(stream), &c);
  } else {
    rc = ns_nerf_forward(a->coarse, nullptr, r.o, r.d, l.z_c, r.view, R, Nc, l.raw_c, stream);
  }
  if (rc != NS_OK) return rc;
  if ((rc = record(a->ev_coarse_end, stream)) != NS_OK) return rc;
  if (!fuse_c) {
    rc = ns_raw2outputs(l.raw_c, l.z_c, r.d, nullptr, R, Nc, a->white_bkgd, nullptr, nullptr, nullptr, nullptr, nullptr, l.w_c,
                        stream);
    if (rc != NS_OK) return rc;
  }
  if (a->Nf == 0) return composite(out, l.raw_c, l.z_c, r.d, R, Nc, a->white_bkgd, stream);   // the coarse pass is the result
  // fine pass (Trainer.py:651-710)
  float* z_f = a->z_dev ? a->z_dev : l.z_f;
  float* raw_f = a->raw_dev ? a->raw_dev : l.raw_f;
  rc = ns_importance_z(l.z_c, l.w_c, R, Nc, a->Nf, a->u_dev, z_f, stream);
  if (rc != NS_OK) return rc;
  if ((rc = record(a->ev_mlp_begin, stream)) != NS_OK) return rc;
  const ns_weights* fine = a->fine ? a->fine : a->coarse;
  if (!chain && ns_nerf_can_composite(fine, Nt)) {
    ns_composite_args c{};
    c.white_bkgd = a->white_bkgd;
    set_outputs(c, out);
    c.max_z_dev = a->max_z_dev; c.max_w_dev = a->max_w_dev; c.max_rgb_dev = a->max_rgb_dev;   // (epilogue argmax)
    rc = ns_nerf_forward_ob16(fine, nullptr, r.o, r.d, z_f, r.view, nullptr, R * Nt, Nt, a->raw_dev, ns::as_stream(stream), &c);
    if (rc != NS_OK) return rc;
    return record(a->ev_mlp_end, stream);
  }
  rc = ns_nerf_forward(fine, nullptr, r.o, r.d, z_f, r.view, R, Nt, raw_f, stream);
  if (rc != NS_OK) return rc;
  if ((rc = record(a->ev_mlp_end, stream)) != NS_OK) return rc;
  Outputs fo = out;
  if (max_sample && !fo.weights) fo.weights = l.w_f;
  rc = composite(fo, raw_f, z_f, r.d, R, Nt, a->white_bkgd, stream);
  if (rc != NS_OK || !max_sample) return rc;
  return ns_argmax_gather(fo.weights, z_f, raw_f, R, Nt, a->max_z_dev, a->max_w_dev, a->max_rgb_dev, stream);
}

int ns_event_create(void** ev) {
  NS_REQUIRE(ev, "null pointer");
  hipEvent_t e;
  NS_HIP(hipEventCreate(&e));
  *ev = e;
  return NS_OK;
}

void ns_event_destroy(void* ev) {
  if (ev) (void)hipEventDestroy(static_cast<hipEvent_t>(ev));
}

int ns_event_record(void* ev, void* stream) {
  NS_REQUIRE(ev, "null event");
  NS_HIP(hipEventRecord(static_cast<hipEvent_t>(ev), ns::as_stream(stream)));
  return NS_OK;
}

int ns_stream_wait_event(void* stream, void* ev) {
  NS_REQUIRE(ev, "null event");
  NS_HIP(hipStreamWaitEvent(ns::as_stream(stream), static_cast<hipEvent_t>(ev), 0));
  return NS_OK;
}

int ns_event_elapsed_ms(void* begin, void* end, float* ms) {
  NS_REQUIRE(begin && end && ms, "null pointer");
  NS_HIP(hipEventSynchronize(static_cast<hipEvent_t>(end)));
  NS_HIP(hipEventElapsedTime(ms, static_cast<hipEvent_t>(begin), static_cast<hipEvent_t>(end)));
  return NS_OK;
}

}  // extern "C"
