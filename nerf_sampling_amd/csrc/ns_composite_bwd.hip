// Backward of alpha compositing (raw2alpha + DepthNetTrainer.raw2outputs: nerf_utils.py:27-42, sampling_trainer.py:153-230)
// and of sample placement (sample_points_around_mean, utils.py:220-244): what torch autograd gives for the reference's
// arithmetic, from the forward's inputs alone.  Nothing of the forward is saved: every kernel re-runs it with the lane layouts
// and building blocks of raw2outputs_kernel (ns_composite_ray.h), so alpha, T and w are the forward's own bits.
//
// Per ray, with keep_i = 1 - alpha_i + 1e-10, T_i = prod_{j<i} keep_j, w_i = alpha_i T_i and g_i = dL/dw_i (the weights'
// own upstream gradient plus what rgb, depth, acc and disp send through sum(w c), sum(w z) and sum(w)):
//   dL/dalpha_k = G_alpha_k + T_k (g_k - U_k),   U_k = sum_{i>k} g_i alpha_i prod_{k<j<i} keep_j,
// computed as the reverse scan  U_k = keep_{k+1} U_{k+1} + g_{k+1} alpha_{k+1}  (a composition of affine maps:
// seg_scan_affine_rev), so nothing is divided by keep_k -- torch's cumprod backward divides, and breaks down as alpha -> 1.
#include "ns_common.h"
#include "ns_composite_ray.h"
#include "ns_place.h"

namespace {

using nscomp::exp_tu;
using nscomp::rcp_tu;

struct UpGrads {                 // upstream gradients, any of them NULL (= that output takes no part in the loss)
  const float* rgb;              // [R,3]
  const float* disp;             // [R]
  const float* acc;              // [R]
  const float* depth;            // [R]
  const float* alphas;           // [R,N]
  const float* weights;          // [R,N]
};

// The per-ray part of the upstream gradient once the ray's totals are known: d rgb_map, and the total gradients of depth_map
// and acc_map (their own, the white background's rgb + (1 - acc), and disp's).
struct RayGrad {
  float gr = 0.f, gg = 0.f, gb = 0.f, gdepth = 0.f, gacc = 0.f;
};
__device__ __forceinline__ RayGrad ray_grad(const UpGrads& G, int64_t r, float depth, float acc, int white_bkgd) {
  RayGrad g;
  if (G.rgb) { g.gr = G.rgb[r * 3]; g.gg = G.rgb[r * 3 + 1]; g.gb = G.rgb[r * 3 + 2]; }
  if (G.depth) g.gdepth = G.depth[r];
  if (G.acc) g.gacc = G.acc[r];
  if (white_bkgd) g.gacc = g.gacc - ((g.gr + g.gg) + g.gb);
  if (G.disp) {
    // disp = 1 / max(1e-10, q), q = depth / (acc + 1e-10): q is the forward's own (nscomp::finish_totals), so the floor is
    // decided on the same bits
    const float den = acc + 1e-10f;
    const float q = depth * rcp_tu(den);
    const float disp = rcp_tu((q != q) ? q : fmaxf(1e-10f, q));
    const float gm = -G.disp[r] * (disp * disp);              // torch's reciprocal backward: -grad * result^2
    // torch.maximum's convention: the whole gradient to the larger operand, half to each on a tie; a NaN q takes all of it
    // (both of maximum's masks are comparisons, false for NaN)
    const float gq = (q > 1e-10f || q != q) ? gm : (q == 1e-10f ? 0.5f * gm : 0.0f);
    g.gdepth = g.gdepth + gq / den;                           // torch's div backward: grad / other ...
    g.gacc = g.gacc + (-gq * depth) / (den * den);            // ... and -grad * self / (other * other)
  }
  return g;
}

// One sample's share of the backward, everything but the reverse scan: recomputed forward values and g (dL/dw).
struct SampleBwd {
  float cr, cg, cb, g, keep;
};
__device__ __forceinline__ SampleBwd sample_pre(const UpGrads& G, const RayGrad& rg, bool ok, int64_t e, float4 q, float zi,
                                                float alpha) {
  SampleBwd s;
  s.cr = s.cg = s.cb = s.g = 0.f;
  s.keep = 1.0f;
  if (ok) {
    s.cr = nscomp::sample_colour(q.x);
    s.cg = nscomp::sample_colour(q.y);
    s.cb = nscomp::sample_colour(q.z);
    const float gw = G.weights ? G.weights[e] : 0.0f;
    s.g = ((gw + ((rg.gr * s.cr + rg.gg * s.cg) + rg.gb * s.cb)) + rg.gdepth * zi) + rg.gacc;
    s.keep = (1.0f - alpha) + 1e-10f;
  }
  return s;
}

// ... and the rest once U (the sum over the later samples) is known: d raw into d_raw[e], the sample's gradient of its distance
// scaled by norm (gdr: what goes to z through z[i+1] - z[i]) and times the raw distance (gn: what goes to |d|).
__device__ __forceinline__ void sample_post(const UpGrads& G, const RayGrad& rg, bool ok, int64_t e, float4 q, float dist_raw,
                                            float norm, float nz, bool has_noise, float T, float w, const SampleBwd& s,
                                            float U, float4* __restrict__ d_raw, float& gdr, float& gn) {
  gdr = 0.f;
  gn = 0.f;
  if (!ok) return;
  // a path no upstream gradient reaches adds nothing, not 0 * (a NaN or inf of the forward): with alphas alone in the loss
  // the transmittance product is not in torch's graph
  float ga = G.alphas ? G.alphas[e] : 0.0f;
  if (G.rgb || G.disp || G.acc || G.depth || G.weights) ga = ga + T * (s.g - U);
  // alpha = 1 - exp(-relu(s) dist): d(relu(s) dist) = ga exp(-relu(s) dist).  relu(NaN) is NaN in torch, and relu's
  // subgradient at 0 is 0 (threshold_backward: the gradient passes where s > 0, and where s is NaN)
  float sg = q.w;
  if (has_noise) sg += nz;
  const float dist = dist_raw * norm;
  const float rl = (sg != sg) ? sg : fmaxf(sg, 0.0f);
  const float t = ga * exp_tu(-rl * dist);
  const float dsig = (sg <= 0.0f) ? 0.0f : t * dist;
  const float ddist = t * rl;
  gdr = ddist * norm;
  gn = ddist * dist_raw;
  if (d_raw) {
    // rgb_map = sum(w c): d c = G_rgb w, then torch's sigmoid backward grad * (1 - y) * y
    float4 o = make_float4(0.f, 0.f, 0.f, dsig);
    if (G.rgb) {
      o.x = ((rg.gr * w) * (1.0f - s.cr)) * s.cr;
      o.y = ((rg.gg * w) * (1.0f - s.cg)) * s.cg;
      o.z = ((rg.gb * w) * (1.0f - s.cb)) * s.cb;
    }
    d_raw[e] = o;
  }
}

// rays_d of ray r: |d| = norm, d|d|/dd = d / |d| (torch's norm backward, zero where the norm is 0)
__device__ __forceinline__ void write_d_rays_d(float* __restrict__ d_rays_d, const float* __restrict__ rays_d, int64_t r,
                                               float norm, float gnorm) {
  const float f = (norm == 0.0f) ? 0.0f : gnorm / norm;
  for (int c = 0; c < 3; ++c) d_rays_d[r * 3 + c] = rays_d[r * 3 + c] * f;
}

// Rays of N <= SW samples: SW lanes per ray, one sample per lane, one pass (the one-chunk layout of raw2outputs_kernel).
template <int SW>
__global__ void __launch_bounds__(256)
raw2outputs_backward_kernel(const float4* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rays_d,
                            const float* __restrict__ noise, int64_t R, int N, int white_bkgd, UpGrads G,
                            float4* __restrict__ d_raw, float* __restrict__ d_z, float* __restrict__ d_rays_d) {
  constexpr int RAYS_PER_BLOCK = 256 / SW;
  const int lane = threadIdx.x & 63, sub = threadIdx.x % SW;
  const int64_t ray_stride = (int64_t)gridDim.x * RAYS_PER_BLOCK;
  const int64_t iters = (R + ray_stride - 1) / ray_stride;     // the same on every lane: the scans need all 64
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t r = it * ray_stride + (int64_t)blockIdx.x * RAYS_PER_BLOCK + threadIdx.x / SW;
    const bool live = r < R, ok = live && sub < N;
    const int64_t e = r * N + sub;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    float zi = 0.f, dist_raw = 0.f, nz = 0.f, norm = 0.f;
    if (live) norm = nscomp::ray_norm(rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]);
    if (ok) {
      q = raw[e];
      zi = z[e];
      dist_raw = (sub < N - 1) ? z[e + 1] - zi : 1e10f;
      if (noise) nz = noise[e];
    }
    // the forward: alpha, T, w of the sample and the ray's totals, as raw2outputs_kernel forms them
    nscomp::RayAccum A;
    float alpha, w, T, disp;
    nscomp::composite_chunk<SW>(A, ok, sub, q, zi, dist_raw, norm, nz, noise != nullptr, alpha, w, &T);
    nscomp::composite_finish<SW>(A, 0, disp, sub);
    const float depth = nscomp::seg_last<SW>(A.depth, lane), acc = nscomp::seg_last<SW>(A.acc, lane);
    RayGrad rg;
    if (live) rg = ray_grad(G, r, depth, acc, white_bkgd);
    const SampleBwd s = sample_pre(G, rg, ok, e, q, zi, alpha);
    // U_k = V_{k+1}, V_i = (f_i o ... o f_{N-1})(0) = b of the reverse scan
    float a = s.keep, b = ok ? s.g * alpha : 0.0f;
    nscomp::seg_scan_affine_rev<SW>(a, b, lane);
    float U = nscomp::from_next_lane(0.0f, b);
    if (sub == SW - 1) U = 0.0f;
    float gdr, gn;
    sample_post(G, rg, ok, e, q, dist_raw, norm, nz, noise != nullptr, T, w, s, U, d_raw, gdr, gn);
    if (d_z) {
      // z[i] enters depth_map (w_i z_i) and the distances z[i+1] - z[i] (the last distance is the constant 1e10)
      float prev = nscomp::from_prev_lane(0.0f, gdr);
      if (sub == 0) prev = 0.0f;
      const float own = ((G.depth || G.disp) ? rg.gdepth * w : 0.0f) - ((sub < N - 1) ? gdr : 0.0f);
      if (ok) d_z[e] = own + prev;
    }
    if (d_rays_d) {
      const float gnorm = nscomp::seg_sum<SW>(gn, lane);
      if (live && sub == SW - 1) write_d_rays_d(d_rays_d, rays_d, r, norm, gnorm);
    }
  }
}

// Rays of N > 64 samples: one wave per ray, 64-sample chunks.  Forward pass in chunk order (the transmittance entering every
// chunk goes to LDS, the totals are raw2outputs_kernel's: add_chunk_totals), then the backward in REVERSE chunk order with U
// carried from chunk to chunk: the reverse scan's carry is V of the chunk's first lane.  z[base] of a chunk also needs gdr of
// the sample before it, which the next chunk processed (the one before) computes: that one value waits in a register.
constexpr int kMaxChunks = 64;              // N <= 4096
__global__ void __launch_bounds__(256)
raw2outputs_backward_chunks_kernel(const float4* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rays_d,
                                   const float* __restrict__ noise, int64_t R, int N, int white_bkgd, UpGrads G,
                                   float4* __restrict__ d_raw, float* __restrict__ d_z, float* __restrict__ d_rays_d) {
  __shared__ float carry_s[4][kMaxChunks];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int64_t iters = (R + nwaves - 1) / nwaves;
  const int nchunks = (N + 63) / 64;
  auto readlane = [](float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); };
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t r = it * nwaves + (int64_t)blockIdx.x * 4 + wv;
    const bool live = r < R;
    float norm = 0.f;
    if (live) norm = nscomp::ray_norm(rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]);
    struct In { bool ok; int64_t e; float4 q; float zi, dist_raw, nz; };
    auto fetch = [&](int base) {
      In x;
      const int i = base + lane;
      x.ok = live && i < N;
      x.e = r * N + i;
      x.q = make_float4(0.f, 0.f, 0.f, 0.f);
      x.zi = x.dist_raw = x.nz = 0.f;
      if (x.ok) {
        x.q = raw[x.e];
        x.zi = z[x.e];
        x.dist_raw = (i < N - 1) ? z[x.e + 1] - x.zi : 1e10f;
        if (noise) x.nz = noise[x.e];
      }
      return x;
    };
    nscomp::RayAccum tot;
    for (int c = 0; c < nchunks; ++c) {
      const In x = fetch(64 * c);
      float alpha, w;
      nscomp::RayAccum A;
      A.carry = tot.carry;
      if (lane == 0) carry_s[wv][c] = tot.carry;
      nscomp::composite_chunk<64>(A, x.ok, lane, x.q, x.zi, x.dist_raw, norm, x.nz, noise != nullptr, alpha, w);
      tot.carry = A.carry;
      nscomp::add_chunk_totals(tot, A);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    RayGrad rg;
    if (live) rg = ray_grad(G, r, tot.depth, tot.acc, white_bkgd);
    float Uc = 0.f, gnorm = 0.f, pend = 0.f;
    int64_t pend_e = -1;
    for (int c = nchunks - 1; c >= 0; --c) {
      const int base = 64 * c;
      const In x = fetch(base);
      nscomp::RayAccum A;
      A.carry = carry_s[wv][c];
      float alpha, w, T;
      nscomp::composite_chunk<64>(A, x.ok, lane, x.q, x.zi, x.dist_raw, norm, x.nz, noise != nullptr, alpha, w, &T);
      const SampleBwd s = sample_pre(G, rg, x.ok, x.e, x.q, x.zi, alpha);
      float a = s.keep, b = x.ok ? s.g * alpha : 0.0f;
      nscomp::seg_scan_affine_rev<64>(a, b, lane);
      const float V = a * Uc + b;                      // (f_i o ... o f_{N-1})(0) with the later chunks folded into Uc
      float U = nscomp::from_next_lane(0.0f, V);
      if (lane == 63) U = Uc;
      Uc = readlane(V, 0);
      float gdr, gn;
      sample_post(G, rg, x.ok, x.e, x.q, x.dist_raw, norm, x.nz, noise != nullptr, T, w, s, U, d_raw, gdr, gn);
      if (d_z) {
        const float own = ((G.depth || G.disp) ? rg.gdepth * w : 0.0f) - ((base + lane < N - 1) ? gdr : 0.0f);
        const float prev = nscomp::from_prev_lane(0.0f, gdr);
        if (lane > 0 && x.ok) d_z[x.e] = own + prev;
        if (lane == 0 && live && pend_e >= 0) d_z[pend_e] = pend + readlane(gdr, 63);   // the chunk after this one
        pend = readlane(own, 0);
        pend_e = x.e;
        if (lane == 0 && live && c == 0) d_z[x.e] = own;
      }
      if (d_rays_d) gnorm = gnorm + nscomp::seg_sum<64>(gn, lane);
    }
    if (d_rays_d && live && lane == 0) write_d_rays_d(d_rays_d, rays_d, r, norm, gnorm);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // this ray's LDS reads are done before the next ray's writes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// N == 1: dists, alphas and weights are [R, 0], rgb_map = sigmoid(raw rgb) (ns_raw2outputs), so only raw's colour channels get
// a gradient; sigma, z and rays_d get zeros (sums over the empty sample axis).
__global__ void __launch_bounds__(256)
raw2outputs_backward_single_kernel(const float4* __restrict__ raw, int64_t R, const float* __restrict__ g_rgb,
                                   float4* __restrict__ d_raw, float* __restrict__ d_z, float* __restrict__ d_rays_d) {
  for (int64_t r = blockIdx.x * (int64_t)256 + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
    if (d_raw) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g_rgb) {
        const float4 q = raw[r];
        const float cr = 1.0f / (1.0f + expf(-q.x)), cg = 1.0f / (1.0f + expf(-q.y)), cb = 1.0f / (1.0f + expf(-q.z));
        o = make_float4((g_rgb[r * 3] * (1.0f - cr)) * cr, (g_rgb[r * 3 + 1] * (1.0f - cg)) * cg,
                        (g_rgb[r * 3 + 2] * (1.0f - cb)) * cb, 0.0f);
      }
      d_raw[r] = o;
    }
    if (d_z) d_z[r] = 0.0f;
    if (d_rays_d) { d_rays_d[r * 3] = 0.0f; d_rays_d[r * 3 + 1] = 0.0f; d_rays_d[r * 3 + 2] = 0.0f; }
  }
}

template <int SW>
void launch_bwd(const float* raw, const float* z, const float* rays_d, const float* noise, int64_t R, int N, int white,
                const UpGrads& G, float* d_raw, float* d_z, float* d_rays_d, hipStream_t s) {
  int64_t grid = ns::cdiv(R, 256 / SW);
  if (grid > 256 * 16) grid = 256 * 16;
  raw2outputs_backward_kernel<SW><<<static_cast<int>(grid), 256, 0, s>>>(
      reinterpret_cast<const float4*>(raw), z, rays_d, noise, R, N, white, G, reinterpret_cast<float4*>(d_raw), d_z, d_rays_d);
}

// d mean of sample_points_around_mean from d z [R,N]: every z[j] is mean + (a constant) before the sort, and the sort only
// permutes, so d mean is the sum over all N samples (the merged mean included) -- times, in the uniform mode, the mask of
// torch.clamp(., 2, 6): the gradient passes where 2 <= z <= 6 before the clip (inclusive bounds; false for NaN, so a NaN mean
// gets 0 there, and the sum of d z in the other modes).
__global__ void __launch_bounds__(256)
place_backward_kernel(int mode, const float* __restrict__ mean, int64_t R, int N, float std_, const float* __restrict__ d_z,
                      float* __restrict__ d_mean) {
  const float step = N > 2 ? (std_ - (-std_)) / static_cast<float>(N - 2) : 0.0f;   // the forward's linspace(-std, std, N - 1)
  for (int64_t r = blockIdx.x * (int64_t)256 + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
    const float m = mean[r];
    float s = 0.0f;
    for (int j = 0; j < N; ++j) {
      const float g = d_z[r * N + j];
      if (mode == NS_MODE_UNIFORM) {
        const float v = nsplace::uniform_z_unclipped(m, std_, step, N - 1, j);
        if (!(v >= 2.0f && v <= 6.0f)) continue;
      }
      s += g;
    }
    d_mean[r] = s;
  }
}

}  // namespace

extern "C" {

int ns_raw2outputs_backward(const float* raw_dev, const float* z_dev, const float* rays_d_dev, const float* noise_dev,
                            int64_t R, int N, int white_bkgd, const float* g_rgb_dev, const float* g_disp_dev,
                            const float* g_acc_dev, const float* g_depth_dev, const float* g_alphas_dev,
                            const float* g_weights_dev, float* d_raw_dev, float* d_z_dev, float* d_rays_d_dev, void* stream) {
  NS_REQUIRE(R >= 0 && N >= 1, "bad shape (N == 0 is handled by the caller)");
  NS_REQUIRE(N <= 64 * kMaxChunks, "the compositing backward takes at most 4096 samples per ray");
  if (R == 0 || !(d_raw_dev || d_z_dev || d_rays_d_dev)) return NS_OK;
  NS_REQUIRE(raw_dev && z_dev && rays_d_dev, "null input");
  NS_REQUIRE((reinterpret_cast<uintptr_t>(raw_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_raw_dev) & 15) == 0,
             "raw and d_raw must be 16-byte aligned");
  hipStream_t s = ns::as_stream(stream);
  if (N == 1) {
    raw2outputs_backward_single_kernel<<<ns::ew_grid(R, 256), 256, 0, s>>>(
        reinterpret_cast<const float4*>(raw_dev), R, g_rgb_dev, reinterpret_cast<float4*>(d_raw_dev), d_z_dev, d_rays_d_dev);
    NS_LAUNCH_CHECK();
    return NS_OK;
  }
  const UpGrads G{g_rgb_dev, g_disp_dev, g_acc_dev, g_depth_dev, g_alphas_dev, g_weights_dev};
#define NS_R2O_BWD(SW) launch_bwd<SW>(raw_dev, z_dev, rays_d_dev, noise_dev, R, N, white_bkgd, G, d_raw_dev, d_z_dev, d_rays_d_dev, s)
  if (N <= 2) NS_R2O_BWD(2);
  else if (N <= 4) NS_R2O_BWD(4);
  else if (N <= 8) NS_R2O_BWD(8);
  else if (N <= 16) NS_R2O_BWD(16);
  else if (N <= 32) NS_R2O_BWD(32);
  else if (N <= 64) NS_R2O_BWD(64);
  else {
    int64_t grid = ns::cdiv(R, 4);
    if (grid > 256 * 16) grid = 256 * 16;
    raw2outputs_backward_chunks_kernel<<<static_cast<int>(grid), 256, 0, s>>>(
        reinterpret_cast<const float4*>(raw_dev), z_dev, rays_d_dev, noise_dev, R, N, white_bkgd, G,
        reinterpret_cast<float4*>(d_raw_dev), d_z_dev, d_rays_d_dev);
  }
#undef NS_R2O_BWD
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_place_samples_backward(int mode, const float* mean_dev, int64_t R, int N, float std_, const float* d_z_dev,
                              float* d_mean_dev, void* stream) {
  NS_REQUIRE(mode == NS_MODE_DEPTH_ONLY || mode == NS_MODE_UNIFORM || mode == NS_MODE_GAUSSIAN, "unknown mode");
  if (mode == NS_MODE_DEPTH_ONLY) N = 1;
  NS_REQUIRE(R >= 0 && N >= 1, "bad shape");
  NS_REQUIRE(mode != NS_MODE_UNIFORM || N >= 2, "uniform mode needs n_samples >= 2");
  if (R == 0) return NS_OK;
  NS_REQUIRE(mean_dev && d_z_dev && d_mean_dev, "null pointer");
  place_backward_kernel<<<ns::ew_grid(R, 256), 256, 0, ns::as_stream(stream)>>>(mode, mean_dev, R, N, std_, d_z_dev, d_mean_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // extern "C"
