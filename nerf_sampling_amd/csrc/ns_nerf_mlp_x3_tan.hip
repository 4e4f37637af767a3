// The one-kernel renderer on an f16x3 field with FORWARD-MODE TANGENTS in the ray's DepthNet depth m (ns_render_rays_fused_tangent).
// In uniform placement every sample depth is m + a constant, clipped to [2, 6], so each composited output of a ray is a function
// of one scalar: the kernel carries d/dm beside every value it computes and returns the six numbers of a ray's Jacobian
// (d rgb / dm, d disp / dm, d depth / dm, d acc / dm).  Nothing per sample is stored.
//
// Shape: the split-fp16 kernel of ns_nerf_mlp_x3.hip (same engine, same weight stream, same bias image) with ONE primal tile of 16
// samples per wave and, as its second register tile, the tangent of that tile: every weight chunk feeds both, so a sample costs
// twice the MFMA work of the forward.  The primal tile runs the generic layer code of the forward (tile by tile the same MFMAs in
// the same order as the generated statements of the production kernel) and is placed and composited by the same epilogue code
// (ns_comp_epilogue.h, groups of 64 samples): its rgb / disp / depth / acc are the forward's bits.
//   placement   z_j = clip(m + c_j, 2, 6): dz_j = 1 where the unclipped depth lies in [2, 6] (bounds included), else 0, and 0
//               for a NaN mean (the mask of ns_place_samples_backward)
//   encoding    d gamma(o + z d) = d dz for the identity features, +-2^k (cos | sin)(2^k p) d dz for the others; the view
//               direction's features are constants
//   field       dh_{l+1} = relu'(pre_l) . (W_l dh_l), no bias; relu'(0) = 0, the mask from the primal tile's pre-activation;
//               the skip layer sees [d gamma, dh], the views layer [dh_feature, 0]; out: d sigma (before its ReLU), d rgb
//               (before the sigmoid)
//   compositing after the group's forward compositing, the rays of the group are walked sample by sample (one lane per ray)
//               with the tangent recurrence of the transmittance, dT_{j+1} = dT_j (1 - alpha_j + 1e-10) - T_j dalpha_j (no
//               division); a ray of several 64-sample chunks carries its walk state from group to group in LDS.
// A product of a value and a tangent is a SELECT on the tangent (tmul): a zero tangent contributes exactly 0, so a ray whose
// samples have no depth tangent (a NaN mean, every sample clipped) has a Jacobian of 0, whatever NaN or inf its forward holds.
#include "ns_common.h"
#include "ns_comp_epilogue.h"
#include "ns_mlp_engine.h"
#include "ns_weights.h"

namespace {

using namespace nsmlp;
using M = Mma16F16x3;
using Block = M::Block;

constexpr int kWaves = 4;
constexpr int kTiles = 1;              // primal tiles per wave (register tile 1 is the tangent of tile 0)
constexpr int kGS = kWaves * kTiles * 16;   // samples per group
using PipeT = Pipe<M, kWaves, 0, kOb16Depth, kOb16Ahead>;
using Rec = nsepi::Records<kTiles, kWaves>;

// the fields place_wave / composite_group read under the names of NerfX3CompArgs, then the tangent outputs
struct TanArgs {
  const char* stream;
  const float* bias;
  uint32_t n_slabs;
  int bias_floats;
  int D;
  uint32_t skip_mask;
  const float* o;
  const float* d;
  const float* viewdirs;
  int64_t S;
  int N;
  int comp;
  int n_shift;
  const float* mean;
  float std_, lin_step;
  int white_bkgd;
  float* rgb; int64_t rgb_stride;
  float* disp; int64_t disp_stride;
  float* weights;
  float* z_out;
  float* pts_out;
  const float* sig_last;
  int m_chunks, sg_groups;
  float fix_thr;
  uint32_t* fix_count;
  float* fix_rec;
  float* max_z;
  float* max_w;
  float* max_rgb;
  float* depth;
  float* acc;
  float* d_rgb;        // [R,3] or NULL
  float* d_disp;       // [R] or NULL
  float* d_depth;      // [R] or NULL
  float* d_acc;        // [R] or NULL
};

// value x tangent, exactly 0 where the tangent is 0 (a select, not a multiply: 0 x inf / NaN of the forward stays out)
__device__ __forceinline__ float tmul(float x, float t) { return t == 0.0f ? 0.0f : x * t; }

// d z_j / d m of sample_points_around_mean("uniform"): the clip's mask on the unclipped depth (false for NaN)
__device__ __forceinline__ float zdot_at(float m, float std_, float step, int steps, int j) {
  const float v = nsplace::uniform_z_unclipped(m, std_, step, steps, j);
  return (v >= 2.0f && v <= 6.0f) ? 1.0f : 0.0f;
}

// Tangent of embedN_16<M, true, 3, L, NKB> (same slots): p the point, pd its tangent; live == false gives zeros.
// d sin(2^k x) = 2^k sin(2^k x + pi / 2), d cos(2^k x) = 2^k sin(2^k x + pi): Trig's quarter-turn offset, one more quarter.
template <int L, int NKB>
__device__ __forceinline__ void embed3_tan16(Block (&out)[NKB], const float (&p)[3], const float (&pd)[3], bool live, int g) {
  constexpr int NC = 3, HALF = 2;
  Rev r[NC];
  static_for<NC>([&](auto i_) { r[decltype(i_)::value] = to_rev(p[decltype(i_)::value]); });
  const bool u = (g >> 1) != 0;
  const int c = g & 1;
  auto dtrig = [&](float hi, float lo, int level, float t) -> float {
    Trig<true> tr(0.0f);
    tr.r.hi = hi; tr.r.lo = lo;
    return (tr(level, c + 1) * __builtin_ldexpf(1.0f, level)) * t;
  };
  static_for<NKB>([&](auto kb_) {
    constexpr int kb = decltype(kb_)::value;
    float x[8];
    static_for<8>([&](auto e_) {
      constexpr int e = decltype(e_)::value;
      constexpr int q0 = 16 * kb + e, q1 = q0 + 8;
      auto value = [&](auto q_) -> float {
        constexpr int j = decltype(q_)::value - NC * L;
        if constexpr (j >= 0 && j < HALF) {
          const float a = pd[j];
          if constexpr (HALF + j < NC) { const float b = pd[HALF + j]; return c ? b : a; }
          else return c ? 0.0f : a;
        } else {
          return 0.0f;
        }
      };
      using Q0 = std::integral_constant<int, q0>;
      using Q1 = std::integral_constant<int, q1>;
      float v;
      if constexpr (q1 < NC * L) {
        const float hi = u ? r[q1 % NC].hi : r[q0 % NC].hi;
        const float lo = u ? r[q1 % NC].lo : r[q0 % NC].lo;
        const float t = u ? pd[q1 % NC] : pd[q0 % NC];
        v = dtrig(hi, lo, u ? q1 / NC : q0 / NC, t);
      } else if constexpr (q0 < NC * L) {
        const float tv = dtrig(r[q0 % NC].hi, r[q0 % NC].lo, q0 / NC, pd[q0 % NC]);
        const float ov = value(Q1{});
        v = u ? ov : tv;
      } else {
        const float a = value(Q0{}), b = value(Q1{});
        v = u ? b : a;
      }
      x[e] = live ? v : 0.0f;
    });
    out[kb] = M::from_f32(x);
  });
}

// the tangent tile's conversion piece: relu'(pre) from the primal tile's pre-activation (ACT == kRelu), no bias
template <int ACT, int SB, int J>
__device__ __forceinline__ void convert_tan_piece16x3(Block& out, const f32x4a& c, const f32x4a& pre) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  float a = c[2 * J], b = c[2 * J + 1];
  if constexpr (ACT == kRelu) { a = pre[2 * J] > 0.0f ? a : 0.0f; b = pre[2 * J + 1] > 0.0f ? b : 0.0f; }
  static_assert(ACT == kRelu || ACT == kNone, "the field has ReLU and linear layers");
  uint32_t h, l;
  M::split2(a, b, h, l);
  u32x4 wh = __builtin_bit_cast(u32x4, out.hi), wl = __builtin_bit_cast(u32x4, out.lo);
  wh[2 * (SB & 1) + J] = h;
  wl[2 * (SB & 1) + J] = l;
  out.hi = __builtin_bit_cast(f16x8, wh);
  out.lo = __builtin_bit_cast(f16x8, wl);
}

// layer_ob16x3<T = 2> (ns_mlp_engine.h) with register tile 0 the primal and tile 1 its tangent: the primal tile is the forward's
// (bias in, ACT on conversion: the same MFMAs in the same order), the tangent tile starts from 0 and is masked by the primal
// pre-activation.  last[0] / last[1]: the raw accumulators of the last sub-block, primal / tangent.
template <int NSB, int NKB, int ACT, class OutT, class InF>
__device__ __forceinline__ void layer_tan16x3(PipeT& pipe, const float* bias_lds, int g, OutT& out, f32x4a (&last)[2], InF&& in) {
  constexpr int T = 2;
  constexpr int CPS = 2 * NKB;
  constexpr int REAL = NSB * CPS;
  constexpr int TOTAL = ob16_chunks(NSB, CPS, PipeT::kDepth);
  constexpr int PIECES = 2 * T;
  constexpr int PPS = (PIECES + CPS - 1) / CPS;
  constexpr int CONV_END = (PIECES + PPS - 1) / PPS;
  constexpr int BIAS_AT = (CPS - 2) > CONV_END ? (CPS - 2) : (CPS - 1);
  const f32x4a zero = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4a c[2][T];
  c[0][0] = *reinterpret_cast<const f32x4a*>(bias_lds + 4 * g);
  c[0][1] = zero;
  stream_chunks<TOTAL>(pipe, [&](auto P_, const typename M::AFrag& frag_ref, auto&& load_next) {
    constexpr int P = decltype(P_)::value;
    if constexpr (P < REAL) {
      constexpr int sb = P / CPS, cc = P % CPS, kc = cc / 2, part = cc % 2, par = sb & 1;
      const typename M::AFrag frag = frag_ref;
      static_for<T>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        const Block& xb = in(t_, std::integral_constant<int, kc>{});
        M::mma(c[par][t], frag, xb.hi);
        if constexpr (part == 0) M::mma(c[par][t], frag, xb.lo);
        if constexpr (t == 0 && sb > 0) {
          static_for<PPS>([&](auto i_) {
            constexpr int piece = cc * PPS + decltype(i_)::value;
            if constexpr (piece < PIECES) {
              if constexpr (piece % T == 0)
                convert_piece16x3<ACT, sb - 1, piece / T>(out[0][(sb - 1) >> 1], c[par ^ 1][0]);
              else
                convert_tan_piece16x3<ACT, sb - 1, piece / T>(out[1][(sb - 1) >> 1], c[par ^ 1][1], c[par ^ 1][0]);
            }
          });
        }
        if constexpr (t == 1) load_next();
        if constexpr (t == T - 1 && cc == BIAS_AT && sb + 1 < NSB) {
          c[par ^ 1][0] = *reinterpret_cast<const f32x4a*>(bias_lds + 16 * (sb + 1) + 4 * g);
          c[par ^ 1][1] = zero;
        }
      });
    } else {
      load_next();
    }
  });
  last[0] = c[(NSB - 1) & 1][0];
  last[1] = c[(NSB - 1) & 1][1];
}
template <int ACT, int NSB, class OutT>
__device__ __forceinline__ void convert_last_tan16x3(OutT& out, const f32x4a (&last)[2]) {
  static_for<2>([&](auto j_) {
    constexpr int j = decltype(j_)::value;
    convert_piece16x3<ACT, NSB - 1, j>(out[0][(NSB - 1) >> 1], last[0]);
    convert_tan_piece16x3<ACT, NSB - 1, j>(out[1][(NSB - 1) >> 1], last[1], last[0]);
  });
}

// LDS records of the tangent pass beyond nsepi::Records, from byte address `base`:
//   float4 per sample of the group {d raw r, g, b, d sigma} | float2 per sample {dz, d dist}, two parities | the walk state of
//   the ray that is open at a group's end (rays of several chunks), kState floats
struct TanRecords {
  static constexpr int kState = 12;
  static constexpr uint32_t kBytes = kGS * 16 + 2 * kGS * 8 + kState * 4 + 16;   // (the state padded to 64 bytes)
  uint32_t base;
  __device__ __forceinline__ nsepi::CrawPtr draw(int i) const {
    return reinterpret_cast<nsepi::CrawPtr>(static_cast<uintptr_t>(base + static_cast<uint32_t>(i) * 16u));
  }
  __device__ __forceinline__ nsepi::CzdPtr dz(uint32_t par, int i) const {
    return reinterpret_cast<nsepi::CzdPtr>(static_cast<uintptr_t>(base + kGS * 16u + (par * kGS + static_cast<uint32_t>(i)) * 8u));
  }
  __device__ __forceinline__ nsepi::CsigPtr state(int k) const {
    return reinterpret_cast<nsepi::CsigPtr>(static_cast<uintptr_t>(base + kGS * 32u + static_cast<uint32_t>(k) * 4u));
  }
};

// a ray's forward quantities and their tangents along the walk
struct Walk {
  float T = 1.0f, dT = 0.0f;
  float r = 0.0f, g = 0.0f, b = 0.0f, depth = 0.0f, acc = 0.0f;
  float dr = 0.0f, dg = 0.0f, db = 0.0f, ddepth = 0.0f, dacc = 0.0f;
  __device__ __forceinline__ void load(const TanRecords& tr) {
    T = *tr.state(0); dT = *tr.state(1);
    r = *tr.state(2); g = *tr.state(3); b = *tr.state(4); depth = *tr.state(5); acc = *tr.state(6);
    dr = *tr.state(7); dg = *tr.state(8); db = *tr.state(9); ddepth = *tr.state(10); dacc = *tr.state(11);
  }
  __device__ __forceinline__ void store(const TanRecords& tr) const {
    *tr.state(0) = T; *tr.state(1) = dT;
    *tr.state(2) = r; *tr.state(3) = g; *tr.state(4) = b; *tr.state(5) = depth; *tr.state(6) = acc;
    *tr.state(7) = dr; *tr.state(8) = dg; *tr.state(9) = db; *tr.state(10) = ddepth; *tr.state(11) = dacc;
  }
};

// samples i0 .. i0 + n - 1 of the group (records of parity par): raw2outputs (sampling_trainer.py:153-230) and its tangent
__device__ __forceinline__ void walk_samples(Walk& W, const Rec& rec, const TanRecords& tr, uint32_t par, int i0, int n) {
  for (int k = 0; k < n; ++k) {
    const int i = i0 + k;
    const nsepi::v4f q = *rec.raw(i), dq = *tr.draw(i);
    const nsepi::v2f zd = *rec.zd(par, i), tz = *tr.dz(par, i);
    const float sg = q.w, dist = zd.y;
    const float rl = (sg != sg) ? sg : fmaxf(sg, 0.0f);
    const float dsg = (sg <= 0.0f) ? 0.0f : dq.w;                     // relu' (threshold_backward: passes for NaN)
    const float ex = nscomp::exp_tu(-rl * dist);
    const float alpha = nscomp::sample_alpha(sg, dist);
    const float dalpha = tmul(ex, tmul(dist, dsg) + tmul(rl, tz.y));
    const float cr = nscomp::sample_colour(q.x), cg = nscomp::sample_colour(q.y), cb = nscomp::sample_colour(q.z);
    const float dcr = tmul(cr * (1.0f - cr), dq.x), dcg = tmul(cg * (1.0f - cg), dq.y), dcb = tmul(cb * (1.0f - cb), dq.z);
    const float w = alpha * W.T;
    const float dw = tmul(W.T, dalpha) + tmul(alpha, W.dT);
    W.r += w * cr; W.g += w * cg; W.b += w * cb; W.depth += w * zd.x; W.acc += w;
    W.dr += tmul(cr, dw) + tmul(w, dcr);
    W.dg += tmul(cg, dw) + tmul(w, dcg);
    W.db += tmul(cb, dw) + tmul(w, dcb);
    W.ddepth += tmul(zd.x, dw) + tmul(w, tz.x);
    W.dacc += dw;
    const float keep = (1.0f - alpha) + 1e-10f;
    W.dT = tmul(keep, W.dT) - tmul(W.T, dalpha);
    W.T = W.T * keep;
  }
}

// the ray's Jacobian from its walk: white background, disp = 1 / max(1e-10, depth / (acc + 1e-10)) (nscomp::finish_totals; on a
// tie of torch.maximum half of the tangent)
__device__ __forceinline__ void write_jacobian(const TanArgs& a, int64_t r, const Walk& W) {
  float dr = W.dr, dg = W.dg, db = W.db;
  if (a.white_bkgd) { dr = dr - W.dacc; dg = dg - W.dacc; db = db - W.dacc; }
  if (a.d_rgb) { a.d_rgb[r * 3] = dr; a.d_rgb[r * 3 + 1] = dg; a.d_rgb[r * 3 + 2] = db; }
  if (a.d_depth) a.d_depth[r] = W.ddepth;
  if (a.d_acc) a.d_acc[r] = W.dacc;
  if (a.d_disp) {
    const float inv = nscomp::rcp_tu(W.acc + 1e-10f);
    const float q = W.depth * inv;
    const float dq = tmul(inv, W.ddepth - tmul(q, W.dacc));
    const float dqm = (q > 1e-10f || q != q) ? dq : (q == 1e-10f ? 0.5f * dq : 0.0f);
    const float disp = nscomp::rcp_tu((q != q) ? q : fmaxf(1e-10f, q));
    a.d_disp[r] = -tmul(disp * disp, dqm);
  }
}

template <int NKB>
__global__ void __launch_bounds__(kWaves * 64)
nerf_mlp_x3_tan_kernel(TanArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NWAVES = kWaves, NSB = 2 * NKB;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int64_t S_ = a.S;
  if (S_ <= 0) return;

  // LDS: [weight ring][bias image][embedding stash: per wave 2 register tiles x 3 blocks x 2 KiB][input staging: per wave
  //      11 x 256 B][nsepi::Records][TanRecords]
  float* bias_lds = reinterpret_cast<float*>(smem + PipeT::kLdsBytes);
  for (int i = threadIdx.x; i < a.bias_floats; i += NWAVES * 64) bias_lds[i] = a.bias[i];
  __syncthreads();

  typedef M::AFrag __attribute__((address_space(3))) * StashPtr;
  const uint32_t lds0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(NS_LDS_PTR(smem)));
  const uint32_t stash_region = lds0 + PipeT::kLdsBytes + ((static_cast<uint32_t>(a.bias_floats) * 4u + 15u) & ~15u);
  const uint32_t stash_base = stash_region + static_cast<uint32_t>(wave) * (2 * 3 * 2048) + static_cast<uint32_t>(lane) * 16u;
  auto stash_at = [&](int t, int b, int half) -> StashPtr {
    return reinterpret_cast<StashPtr>(static_cast<uintptr_t>(stash_base + ((t * 3 + b) * 2 + half) * 1024));
  };
  auto stash_put = [&](int t, int b, const Block& v) { *stash_at(t, b, 0) = v.hi; *stash_at(t, b, 1) = v.lo; };
  auto stash_get = [&](int t, int b) -> Block { Block v; v.hi = *stash_at(t, b, 0); v.lo = *stash_at(t, b, 1); return v; };
  constexpr uint32_t kStageRows = 11;
  const uint32_t stage_base = stash_region + NWAVES * (2 * 3 * 2048) + static_cast<uint32_t>(wave) * (kStageRows * 256);
  const Rec rec{stash_region + NWAVES * (2 * 3 * 2048) + NWAVES * (kStageRows * 256)};
  const TanRecords tr{rec.base + Rec::kBytes};

  PipeT ring;
  ring.init(a.stream, smem, a.n_slabs, wave, lane);

  const int64_t n_groups = (S_ + kGS - 1) / kGS;
  auto sample_of = [&](int64_t grp, int l16, bool& valid) -> int64_t {
    const int64_t sidx = (grp * NWAVES + wave) * 16 + l16;
    valid = sidx < S_;
    return valid ? sidx : S_ - 1;
  };
  // the next group's inputs by LDS-DMA (ns_nerf_mlp_x3.hip): o 0..2, d 3..5, the ray's DepthNet depth 6, view direction 7..9
  // (lanes 16 .. 63 re-fetch the values of lanes 0 .. 15, harmlessly)
  auto prefetch = [&](int64_t grp) {
    bool valid;
    const int64_t sidx = sample_of(grp, lane & 15, valid);
    const int64_t ray = S_ <= 0x7fffffff ? static_cast<int64_t>(static_cast<uint32_t>(sidx) / static_cast<uint32_t>(a.N))
                                          : sidx / a.N;
#pragma unroll
    for (int c = 0; c < 3; ++c) { lds_dma4(a.o + ray * 3 + c, stage_base + c * 256); lds_dma4(a.d + ray * 3 + c, stage_base + (3 + c) * 256); }
    lds_dma4(a.mean + ray, stage_base + 6 * 256);
#pragma unroll
    for (int c = 0; c < 3; ++c) lds_dma4(a.viewdirs + ray * 3 + c, stage_base + (7 + c) * 256);
  };
  auto staged = [&](int slot, int i) -> float {
    return *reinterpret_cast<const float __attribute__((address_space(3)))*>(static_cast<uintptr_t>(stage_base + slot * 256 + i * 4));
  };

  // runs of sg consecutive groups (a ray of m = N / 64 chunks is one run: group gi of the run is its chunk gi), then a jump
  const int sg = a.sg_groups > 1 ? a.sg_groups : 1;
  const int64_t grp0 = static_cast<int64_t>(blockIdx.x) * sg;
  prefetch(grp0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uint32_t par = 0;
  int gi = 0;
  for (int64_t grp = grp0, nxt_grp = 0; grp < n_groups; grp = nxt_grp, gi = (gi + 1 == sg ? 0 : gi + 1), par ^= 1u) {
    nxt_grp = gi + 1 == sg ? grp + static_cast<int64_t>(gridDim.x - 1) * sg + 1 : grp + 1;
    Block xe[2][2];   // embedded point and its tangent
    asm volatile("" ::: "memory");
    nsepi::place_wave(a, rec, staged, grp, gi, par, wave);
    {
      // the tile: sample n of the wave (position j in its ray)
      const int ig = wave * 16 + n;
      const int j = a.m_chunks ? gi * kGS + ig : (ig & (a.N - 1));
      const float m = staged(6, n);
      const float zz = (*rec.zd(par, ig)).x;
      const float zd0 = zdot_at(m, a.std_, a.lin_step, a.N - 1, j);
      const float zd1 = zdot_at(m, a.std_, a.lin_step, a.N - 1, j + 1);
      float p[3], pd[3], v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { p[c] = staged(c, n) + staged(3 + c, n) * zz; pd[c] = staged(3 + c, n) * zd0; }
      if (g == 0) {   // {dz, d dist}: d dist = (dz_{j+1} - dz_j) |d|, 0 for the last sample (its 1e10 is a constant)
        const float nrm = nscomp::ray_norm(staged(3, n), staged(4, n), staged(5, n));
        *tr.dz(par, ig) = nsepi::v2f{zd0, j < a.N - 1 ? tmul(nrm, zd1 - zd0) : 0.0f};
      }
      embedN_16<M, true, 3, 10, 2>(xe[0], p, g);
      embed3_tan16<10, 2>(xe[1], p, pd, zd0 != 0.0f, g);
      Block ve[1];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = staged(7 + c, n);
      embedN_16<M, true, 3, 4, 1>(ve, v, g);
      stash_put(0, 0, xe[0][0]); stash_put(0, 1, xe[0][1]); stash_put(0, 2, ve[0]);
      stash_put(1, 0, xe[1][0]); stash_put(1, 1, xe[1][1]);
    }

    const float* bias = bias_lds;
    Block hA[2][NKB], hB[2][NKB];
    f32x4a last[2];
    auto in_x = [&](auto t_, auto kb_) -> const Block& { return xe[decltype(t_)::value][decltype(kb_)::value]; };
    auto in_A = [&](auto t_, auto kb_) -> const Block& { return hA[decltype(t_)::value][decltype(kb_)::value]; };
    auto in_B = [&](auto t_, auto kb_) -> const Block& { return hB[decltype(t_)::value][decltype(kb_)::value]; };
    Block xs[2][2];
    auto load_xs = [&] {
      static_for<2>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        xs[t][0] = stash_get(t, 0); xs[t][1] = stash_get(t, 1);
      });
    };
    auto in_xA = [&](auto t_, auto kb_) -> const Block& {
      constexpr int kb = decltype(kb_)::value;
      if constexpr (kb < 2) return xs[decltype(t_)::value][kb]; else return hA[decltype(t_)::value][kb - 2];
    };
    auto in_xB = [&](auto t_, auto kb_) -> const Block& {
      constexpr int kb = decltype(kb_)::value;
      if constexpr (kb < 2) return xs[decltype(t_)::value][kb]; else return hB[decltype(t_)::value][kb - 2];
    };

    layer_tan16x3<NSB, 2, kRelu>(ring, bias, g, hA, last, in_x); convert_last_tan16x3<kRelu, NSB>(hA, last); bias += NSB * 16;
    prefetch(nxt_grp);
    int l = 1;
    for (; l + 1 < a.D; l += 2) {
      if ((a.skip_mask >> (l - 1)) & 1u) { load_xs(); layer_tan16x3<NSB, NKB + 2, kRelu>(ring, bias, g, hB, last, in_xA); }
      else layer_tan16x3<NSB, NKB, kRelu>(ring, bias, g, hB, last, in_A);
      convert_last_tan16x3<kRelu, NSB>(hB, last); bias += NSB * 16;
      if ((a.skip_mask >> l) & 1u) { load_xs(); layer_tan16x3<NSB, NKB + 2, kRelu>(ring, bias, g, hA, last, in_xB); }
      else layer_tan16x3<NSB, NKB, kRelu>(ring, bias, g, hA, last, in_B);
      convert_last_tan16x3<kRelu, NSB>(hA, last); bias += NSB * 16;
    }
    if (l < a.D) {
      if ((a.skip_mask >> (l - 1)) & 1u) { load_xs(); layer_tan16x3<NSB, NKB + 2, kRelu>(ring, bias, g, hB, last, in_xA); }
      else layer_tan16x3<NSB, NKB, kRelu>(ring, bias, g, hB, last, in_A);
      convert_last_tan16x3<kRelu, NSB>(hB, last); bias += NSB * 16;
      static_for<2>([&](auto t_) { static_for<NKB>([&](auto b_) { hA[decltype(t_)::value][decltype(b_)::value] = hB[decltype(t_)::value][decltype(b_)::value]; }); });
    }
    // views o feature on cat[h, dirs27] (tangent: [dh, 0]) with alpha_linear as row 0 of the last sub-block; then rgb
    Block vs[2];
    vs[0] = stash_get(0, 2);
    vs[1].hi = f16x8{}; vs[1].lo = f16x8{};
    auto in_Av = [&](auto t_, auto kb_) -> const Block& {
      constexpr int kb = decltype(kb_)::value;
      if constexpr (kb < NKB) return hA[decltype(t_)::value][kb]; else return vs[decltype(t_)::value];
    };
    layer_tan16x3<NSB / 2 + 1, NKB + 1, kRelu>(ring, bias, g, hB, last, in_Av); bias += (NSB / 2 + 1) * 16;
    const float sigma = last[0][0], dsigma = last[1][0];
    layer_tan16x3<1, NKB / 2, kNone>(ring, bias, g, hA, last, in_B);

    const int le = nsepi::opaque_lane();
    if (le < 16) {
      *rec.raw(wave * 16 + le) = nsepi::v4f{last[0][0], last[0][1], last[0][2], sigma};
      *tr.draw(wave * 16 + le) = nsepi::v4f{last[1][0], last[1][1], last[1][2], dsigma};
    }
    nsepi::composite_group(a, rec, true, grp, gi, par, wave, le);   // the forward's outputs (barrier inside)

    // the tangents: wave 0 walks the group's rays, one lane per ray (every wave's records are in LDS: composite_group's barrier)
    if (wave == 0) {
      const int64_t s0 = grp * kGS;
      if (a.m_chunks) {                            // the group is chunk gi of ray grp / m
        if (le == 0) {
          Walk W;
          if (gi > 0) W.load(tr);
          walk_samples(W, rec, tr, par, 0, kGS);
          if (gi + 1 == a.m_chunks) {
            if (s0 < S_) write_jacobian(a, grp / a.m_chunks, W);
          } else {
            W.store(tr);
          }
        }
      } else {
        const int rays = kGS >> a.n_shift;
        if (le < rays && s0 + static_cast<int64_t>(le) * a.N < S_) {
          Walk W;
          walk_samples(W, rec, tr, par, le * a.N, a.N);
          write_jacobian(a, (s0 >> a.n_shift) + le, W);
        }
      }
    }
  }
  ring.finish();
}

int x3_program_slabs(int W, int D, uint32_t skip_mask) {   // with view directions (ns_nerf_mlp_x3.hip)
  const int NSB = W / 16, NKB = W / 32, dp = kOb16Depth;
  int n = ob16_layer_slabs(NSB, 2 * 2, dp);
  for (int l = 1; l < D; ++l) n += ob16_layer_slabs(NSB, 2 * (((skip_mask >> (l - 1)) & 1u) ? NKB + 2 : NKB), dp);
  return n + ob16_layer_slabs(NSB / 2 + 1, 2 * (NKB + 1), dp) + ob16_layer_slabs(1, 2 * (NKB / 2), dp);
}

size_t tan_lds_bytes(int bias_floats) {
  return static_cast<size_t>(PipeT::kLdsBytes) + ((static_cast<size_t>(bias_floats) * 4 + 15) & ~size_t(15)) +
         static_cast<size_t>(kWaves) * 2 * 3 * 2048 + static_cast<size_t>(kWaves) * 11 * 256 + Rec::kBytes + TanRecords::kBytes;
}

template <int NKB>
int launch_tan(TanArgs& a, hipStream_t stream) {
  const size_t lds = tan_lds_bytes(a.bias_floats);
  if (lds > 160 * 1024) {
    ns::set_error("ns_render_rays_fused_tangent: %zu bytes of LDS needed (too deep a network for the resident bias image)", lds);
    return NS_E_UNSUPPORTED;
  }
  auto kern = nerf_mlp_x3_tan_kernel<NKB>;
  NS_HIP(ns::ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds));
  const int64_t n_groups = (a.S + kGS - 1) / kGS;
  int cus = ns::cu_count();
  if (cus <= 0) cus = 256;
  a.sg_groups = nsepi::run_groups(kGS, a.m_chunks, a.N);
  const int64_t n_runs = (n_groups + a.sg_groups - 1) / a.sg_groups;
  const int grid = static_cast<int>(n_runs < cus ? n_runs : cus);
  kern<<<grid, kWaves * 64, lds, stream>>>(a);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // namespace

// called by ns_render_rays_fused_tangent (ns_render.cpp), which has checked the handle (ns_render_tangent_supported) and the
// outputs: rays (o, d, view), the DepthNet depth of every ray in comp->mean_dev, the forward's per-ray outputs in comp
int ns_nerf_forward_x3_tangent(const ns_weights* net, const float* o_dev, const float* d_dev, const float* viewdirs_dev, int64_t R,
                               int N, const ns_composite_args* comp, float* d_rgb, float* d_disp, float* d_depth, float* d_acc,
                               hipStream_t stream) {
  if (x3_program_slabs(net->width, net->depth, net->skip_mask) != static_cast<int>(net->n_slabs)) {
    ns::set_error("ns_render_rays_fused_tangent: packed stream has %u slabs, kernel program expects %d", net->n_slabs,
                  x3_program_slabs(net->width, net->depth, net->skip_mask));
    return NS_E_INVALID;
  }
  TanArgs a{};
  a.stream = static_cast<const char*>(net->stream_dev);
  a.bias = net->bias_dev; a.n_slabs = net->n_slabs; a.bias_floats = net->bias_floats;
  a.D = net->depth; a.skip_mask = net->skip_mask;
  a.o = o_dev; a.d = d_dev; a.viewdirs = viewdirs_dev;
  a.S = R * N; a.N = N;
  nsepi::set_comp_args(a, comp, N);
  a.d_rgb = d_rgb; a.d_disp = d_disp; a.d_depth = d_depth; a.d_acc = d_acc;
  return net->width == 256 ? launch_tan<8>(a, stream) : launch_tan<4>(a, stream);
}
