// The one-kernel renderer on an f16 field with FORWARD-MODE TANGENTS in the ray's DepthNet depth m: the 16-bit
// counterpart of ns_nerf_mlp_x3_tan.hip (ns_render_rays_fused_tangent dispatches on the handle's dtype).  In uniform placement
// every sample depth is m + a constant, clipped to [2, 6], so the composited outputs of a ray are functions of one scalar; the
// kernel carries d/dm beside every value and returns the six numbers of a ray's Jacobian (d rgb / dm, d disp / dm, d depth / dm,
// d acc / dm).  Nothing per sample is stored.
//
// Shape: the engine, weight stream and bias image of the 16-bit forward (ns_nerf_mlp_ob16.hip) with TWO primal tiles of 16
// samples per wave and, as register tiles 2 and 3, their tangents: every weight chunk feeds all four, the register footprint of the
// forward's four-tile generic kernel.  The primal tiles run the compiled layer code of the forward (tile by tile the same MFMAs in
// the same order; the generated production statements are bit-identical to it) and the forward's placement and compositing
// (ns_comp_epilogue.h, groups of 128 samples): their rgb / disp / depth / acc are the forward's bits.  The tangent tiles are held
// in the field's own 16-bit operand type, so J is the derivative carried through the field's 16-bit arithmetic:
//   placement   z_j = clip(m + c_j, 2, 6): dz_j = 1 where the unclipped depth lies in [2, 6] (bounds included), else 0, and 0
//               for a NaN mean
//   encoding    d gamma(o + z d) = d dz for the identity features, +-2^k (cos | sin)(2^k p) d dz for the others (v_sin, as the
//               forward's encoding); the view direction's features are constants
//   field       dh_{l+1} = relu'(pre_l) . (W_l dh_l), no bias; relu'(0) = 0, the mask from the primal tile's fp32 pre-activation;
//               the skip layer sees [d gamma, dh], the views layer [dh_feature, 0]; out: d sigma (before its ReLU), d rgb
//               (before the sigmoid)
//   compositing after the group's forward compositing, wave 0 walks the group's rays sample by sample (one lane per ray) with
//               dT_{j+1} = dT_j (1 - alpha_j + 1e-10) - T_j dalpha_j; a ray of several chunks carries its walk state in LDS.
// A product of a value and a tangent is a SELECT on the tangent (tmul): a zero tangent contributes exactly 0, so a ray whose
// samples have no depth tangent (a NaN mean, every sample clipped) has a Jacobian of 0, whatever NaN or inf its forward holds.
// The walk, its records and the Jacobian's finish are those of ns_nerf_mlp_x3_tan.hip, repeated here for a 128-sample group.
#include "ns_common.h"
#include "ns_comp_epilogue.h"
#include "ns_mlp_engine.h"
#include "ns_weights.h"

namespace {

using namespace nsmlp;

constexpr int kWaves = 4;
constexpr int kTiles = 2;                   // primal tiles per wave; register tile kTiles + t is the tangent of tile t
constexpr int kRT = 2 * kTiles;             // register tiles per wave
constexpr int kGS = kWaves * kTiles * 16;   // samples per group
template <class M>
using PipeOf = Pipe<M, kWaves, 0, kOb16Depth, kOb16Ahead>;
using Rec = nsepi::Records<kTiles, kWaves>;

// the fields place_wave / composite_group read under the names of Nerf16Args, then the tangent outputs
struct Tan16Args {
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

// Tangent of embed3_16<M, false, L, NKB> (same slots): p the point, pd its tangent; live == false gives zeros.
// d sin(2^k x) = 2^k sin(2^k x + pi / 2), d cos(2^k x) = 2^k sin(2^k x + pi): Trig's quarter-turn offset, one more quarter.
template <class M, int L, int NKB>
__device__ __forceinline__ void embed3_tan16b(typename M::Block (&out)[NKB], const float (&p)[3], const float (&pd)[3], bool live,
                                              int g) {
  const Rev r0 = to_rev(p[0]), r1 = to_rev(p[1]), r2 = to_rev(p[2]);
  const bool u = (g >> 1) != 0;
  const int c = g & 1;
  auto dtrig = [&](float hi, float lo, int level, float t) -> float {
    Trig<false> tr(0.0f);
    tr.r.hi = hi; tr.r.lo = lo;
    return (tr(level, c + 1) * __builtin_ldexpf(1.0f, level)) * t;
  };
  static_for<NKB>([&](auto kb_) {
    constexpr int kb = decltype(kb_)::value;
    float x[8];
    static_for<8>([&](auto e_) {
      constexpr int e = decltype(e_)::value;
      constexpr int q0 = 16 * kb + e, q1 = q0 + 8;
      auto value = [&](auto q_) -> float {               // the identity slots: x0 / x2, x1 / pad
        constexpr int q = decltype(q_)::value;
        if constexpr (q == 3 * L) return c ? pd[2] : pd[0];
        else if constexpr (q == 3 * L + 1) return c ? 0.0f : pd[1];
        else return 0.0f;
      };
      auto comp_hi = [&](auto q_) -> float { constexpr int k = decltype(q_)::value % 3; return k == 0 ? r0.hi : (k == 1 ? r1.hi : r2.hi); };
      auto comp_lo = [&](auto q_) -> float { constexpr int k = decltype(q_)::value % 3; return k == 0 ? r0.lo : (k == 1 ? r1.lo : r2.lo); };
      using Q0 = std::integral_constant<int, q0>;
      using Q1 = std::integral_constant<int, q1>;
      float v;
      if constexpr (q1 < 3 * L) {
        const float hi = u ? comp_hi(Q1{}) : comp_hi(Q0{});
        const float lo = u ? comp_lo(Q1{}) : comp_lo(Q0{});
        const float t = u ? pd[q1 % 3] : pd[q0 % 3];
        v = dtrig(hi, lo, u ? q1 / 3 : q0 / 3, t);
      } else if constexpr (q0 < 3 * L) {
        const float tv = dtrig(comp_hi(Q0{}), comp_lo(Q0{}), q0 / 3, pd[q0 % 3]);
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
template <class M, int ACT, int SB, int J>
__device__ __forceinline__ void convert_tan_piece16(typename M::Block& out, const f32x4a& c, const f32x4a& pre) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  static_assert(ACT == kRelu || ACT == kNone, "the field has ReLU and linear layers");
  float a = c[2 * J], b = c[2 * J + 1];
  if constexpr (ACT == kRelu) { a = pre[2 * J] > 0.0f ? a : 0.0f; b = pre[2 * J + 1] > 0.0f ? b : 0.0f; }
  u32x4 w = __builtin_bit_cast(u32x4, out.v);
  w[2 * (SB & 1) + J] = M::template pack2<false>(a, b);
  out.v = __builtin_bit_cast(typename M::AFrag, w);
}

// layer_ob16<M, T = 4> (ns_mlp_engine.h) with register tiles 0, 1 the primal and 2, 3 their tangents: the primal tiles are the
// forward's (bias in, ACT on conversion: the same MFMAs in the same order), the tangent tiles start from 0 and are masked by their
// primal tile's pre-activation.  last[t]: the raw accumulators of the last sub-block.
template <class M, int NSB, int NKB, int ACT, class OutT, class InF>
__device__ __forceinline__ void layer_tan16(PipeOf<M>& pipe, const float* bias_lds, int g, OutT& out, f32x4a (&last)[kRT], InF&& in) {
  constexpr int T = kRT;
  constexpr int REAL = NSB * NKB;
  constexpr int TOTAL = ob16_chunks(NSB, NKB, PipeOf<M>::kDepth);
  constexpr int PIECES = 2 * T;
  constexpr int PPS = (PIECES + NKB - 1) / NKB;
  constexpr int CONV_END = (PIECES + PPS - 1) / PPS;
  constexpr int BIAS_AT = (NKB - 2) > CONV_END ? (NKB - 2) : (NKB - 1);
  const f32x4a zero = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4a c[2][T];
  {
    const f32x4a b0 = *reinterpret_cast<const f32x4a*>(bias_lds + 4 * g);
    static_for<T>([&](auto t_) { c[0][decltype(t_)::value] = decltype(t_)::value < kTiles ? b0 : zero; });
  }
  stream_chunks<TOTAL>(pipe, [&](auto P_, const typename M::AFrag& frag_ref, auto&& load_next) {
    constexpr int P = decltype(P_)::value;
    if constexpr (P < REAL) {
      constexpr int sb = P / NKB, kc = P % NKB, par = sb & 1;
      const typename M::AFrag frag = frag_ref;
      static_for<T>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        M::mma(c[par][t], frag, in(t_, std::integral_constant<int, kc>{}));
        if constexpr (t == 0 && sb > 0) {
          static_for<PPS>([&](auto i_) {
            constexpr int piece = kc * PPS + decltype(i_)::value;
            if constexpr (piece < PIECES) {
              constexpr int pt = piece % T;
              if constexpr (pt < kTiles)
                convert_piece16<M, ACT, sb - 1, piece / T>(out[pt][(sb - 1) >> 1], c[par ^ 1][pt]);
              else
                convert_tan_piece16<M, ACT, sb - 1, piece / T>(out[pt][(sb - 1) >> 1], c[par ^ 1][pt], c[par ^ 1][pt - kTiles]);
            }
          });
        }
        if constexpr (t == 1) load_next();
        if constexpr (t == 2 && kc == BIAS_AT && sb + 1 < NSB) {
          const f32x4a bn = *reinterpret_cast<const f32x4a*>(bias_lds + 16 * (sb + 1) + 4 * g);
          static_for<T>([&](auto u_) { c[par ^ 1][decltype(u_)::value] = decltype(u_)::value < kTiles ? bn : zero; });
        }
      });
    } else {
      load_next();
    }
  });
  static_for<T>([&](auto t_) { last[decltype(t_)::value] = c[(NSB - 1) & 1][decltype(t_)::value]; });
}
template <class M, int ACT, int NSB, class OutT>
__device__ __forceinline__ void convert_last_tan16(OutT& out, const f32x4a (&last)[kRT]) {
  static_for<kTiles>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<2>([&](auto j_) {
      constexpr int j = decltype(j_)::value;
      convert_piece16<M, ACT, NSB - 1, j>(out[t][(NSB - 1) >> 1], last[t]);
      convert_tan_piece16<M, ACT, NSB - 1, j>(out[kTiles + t][(NSB - 1) >> 1], last[kTiles + t], last[t]);
    });
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
__device__ __forceinline__ void write_jacobian(const Tan16Args& a, int64_t r, const Walk& W) {
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

template <class M, int NKB>
__global__ void __launch_bounds__(kWaves * 64)
nerf_tan16_kernel(Tan16Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NWAVES = kWaves, NSB = 2 * NKB;
  using Block = typename M::Block;
  using PipeT = PipeOf<M>;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int64_t S_ = a.S;
  if (S_ <= 0) return;

  // LDS: [weight ring][bias image][embedding stash: per wave 4 register tiles x 3 blocks x 1 KiB][input staging: per wave 11
  //      rows of 16 kTiles floats][nsepi::Records][TanRecords]
  float* bias_lds = reinterpret_cast<float*>(smem + PipeT::kLdsBytes);
  for (int i = threadIdx.x; i < a.bias_floats; i += NWAVES * 64) bias_lds[i] = a.bias[i];
  __syncthreads();

  typedef typename M::AFrag __attribute__((address_space(3))) * StashPtr;
  const uint32_t lds0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(NS_LDS_PTR(smem)));
  const uint32_t stash_region = lds0 + PipeT::kLdsBytes + ((static_cast<uint32_t>(a.bias_floats) * 4u + 15u) & ~15u);
  const uint32_t stash_base = stash_region + static_cast<uint32_t>(wave) * (kRT * 3 * 1024) + static_cast<uint32_t>(lane) * 16u;
  auto stash_at = [&](int t, int b) -> StashPtr {
    return reinterpret_cast<StashPtr>(static_cast<uintptr_t>(stash_base + (t * 3 + b) * 1024));
  };
  auto stash_put = [&](int t, int b, const Block& v) { *stash_at(t, b) = v.v; };
  auto stash_get = [&](int t, int b) -> Block { Block v; v.v = *stash_at(t, b); return v; };
  // staging: value slot k (0..10) of sample j (0 .. 16 kTiles - 1) of this wave's group at stage_base + k * kStageRow + j * 4 (a
  // row is one LDS-DMA of the 64 lanes: 4 bytes each)
  constexpr uint32_t kStageRow = 256, kStageRows = 11;
  const uint32_t stage_base = stash_region + NWAVES * (kRT * 3 * 1024) + static_cast<uint32_t>(wave) * (kStageRows * kStageRow);
  const Rec rec{stash_region + NWAVES * (kRT * 3 * 1024) + NWAVES * (kStageRows * kStageRow)};
  const TanRecords tr{rec.base + Rec::kBytes};

  PipeT ring;
  ring.init(a.stream, smem, a.n_slabs, wave, lane);

  const int64_t n_groups = (S_ + kGS - 1) / kGS;
  auto sample_of = [&](int64_t grp, int t, int l16, bool& valid) -> int64_t {
    const int64_t sidx = ((grp * NWAVES + wave) * kTiles + t) * 16 + l16;
    valid = sidx < S_;
    return valid ? sidx : S_ - 1;
  };
  // the next group's inputs by LDS-DMA (ns_nerf_mlp_ob16.hip): o 0..2, d 3..5, the ray's DepthNet depth 6, view direction 7..9;
  // lanes 16 t .. 16 t + 15 fetch tile t (lanes past the last tile re-fetch it, harmlessly)
  auto prefetch = [&](int64_t grp) {
    bool valid;
    const int tl = lane >> 4;
    const int64_t sidx = sample_of(grp, tl < kTiles ? tl : kTiles - 1, lane & 15, valid);
    const int64_t ray = S_ <= 0x7fffffff ? static_cast<int64_t>(static_cast<uint32_t>(sidx) / static_cast<uint32_t>(a.N))
                                          : sidx / a.N;
    auto put = [&](int slot, const float* src) { lds_dma4(src, stage_base + slot * kStageRow); };
#pragma unroll
    for (int c = 0; c < 3; ++c) { put(c, a.o + ray * 3 + c); put(3 + c, a.d + ray * 3 + c); }
    put(6, a.mean + ray);
#pragma unroll
    for (int c = 0; c < 3; ++c) put(7 + c, a.viewdirs + ray * 3 + c);
  };
  auto staged_at = [&](int slot, int i) -> float {
    return *reinterpret_cast<const float __attribute__((address_space(3)))*>(static_cast<uintptr_t>(stage_base + slot * kStageRow + i * 4));
  };

  // runs of sg consecutive groups (whole rays when a ray spans several chunks), then a jump
  const int sg = a.sg_groups > 1 ? a.sg_groups : 1;
  const int64_t grp0 = static_cast<int64_t>(blockIdx.x) * sg;
  prefetch(grp0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uint32_t par = 0;
  int gi = 0;
  for (int64_t grp = grp0, nxt_grp = 0; grp < n_groups; grp = nxt_grp, gi = (gi + 1 == sg ? 0 : gi + 1), par ^= 1u) {
    nxt_grp = gi + 1 == sg ? grp + static_cast<int64_t>(gridDim.x - 1) * sg + 1 : grp + 1;
    Block xe[kRT][2];   // embedded points (tiles 0, 1) and their tangents (tiles 2, 3)
    // non-finite inputs: written as NaN, as the forward does (ns_nerf_mlp_ob16.hip: the packed-int16 ReLU would drop the negative
    // NaNs of the matrix cores)
    uint32_t bad = 0;
    auto finite = [](float v) { return __builtin_fabsf(v) < __builtin_inff(); };
    asm volatile("" ::: "memory");
    nsepi::place_wave(a, rec, staged_at, grp, gi, par, wave);
    {
      const int jg0 = a.m_chunks ? (gi * kGS) % a.N : 0;
      float P[kTiles][3], PD[kTiles][3], V[kTiles][3], ZD[kTiles];
      static_for<kTiles>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        const int ig = (wave * kTiles + t) * 16 + n;
        int j = a.m_chunks ? jg0 + ig : (ig & (a.N - 1));
        if (a.m_chunks && j >= a.N) j -= a.N;                        // (jg0 + ig < N + kGS <= 2 N)
        const float m = staged_at(6, t * 16 + n);
        const float zz = (*rec.zd(par, ig)).x;
        ZD[t] = zdot_at(m, a.std_, a.lin_step, a.N - 1, j);
        static_for<3>([&](auto c_) {
          constexpr int c = decltype(c_)::value;
          P[t][c] = staged_at(c, t * 16 + n) + staged_at(3 + c, t * 16 + n) * zz;
          PD[t][c] = staged_at(3 + c, t * 16 + n) * ZD[t];
          V[t][c] = staged_at(7 + c, t * 16 + n);
        });
        if (g == 0) {   // {dz, d dist}: d dist = (dz_{j+1} - dz_j) |d|, 0 for the last sample (its 1e10 is a constant)
          const float zd1 = zdot_at(m, a.std_, a.lin_step, a.N - 1, j + 1);
          const float nrm = nscomp::ray_norm(staged_at(3, t * 16 + n), staged_at(4, t * 16 + n), staged_at(5, t * 16 + n));
          *tr.dz(par, ig) = nsepi::v2f{ZD[t], j < a.N - 1 ? tmul(nrm, zd1 - ZD[t]) : 0.0f};
        }
      });
      asm volatile("" ::: "memory");   // the staged reads above, then the stash writes (two LDS regions)
      static_for<kTiles>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        const bool ok = finite(P[t][0]) && finite(P[t][1]) && finite(P[t][2]) && finite(V[t][0]) && finite(V[t][1]) &&
                        finite(V[t][2]);
        if (!ok) bad |= 1u << t;
        embed3_16<M, false, 10, 2>(xe[t], P[t][0], P[t][1], P[t][2], g);
        embed3_tan16b<M, 10, 2>(xe[kTiles + t], P[t], PD[t], ZD[t] != 0.0f, g);
        Block ve[1];
        embed3_16<M, false, 4, 1>(ve, V[t][0], V[t][1], V[t][2], g);
        stash_put(t, 0, xe[t][0]); stash_put(t, 1, xe[t][1]); stash_put(t, 2, ve[0]);
        stash_put(kTiles + t, 0, xe[kTiles + t][0]); stash_put(kTiles + t, 1, xe[kTiles + t][1]);
      });
    }

    const float* bias = bias_lds;
    Block hA[kRT][NKB], hB[kRT][NKB];
    f32x4a last[kRT];
    auto in_x = [&](auto t_, auto kb_) -> const Block& { return xe[decltype(t_)::value][decltype(kb_)::value]; };
    auto in_A = [&](auto t_, auto kb_) -> const Block& { return hA[decltype(t_)::value][decltype(kb_)::value]; };
    auto in_B = [&](auto t_, auto kb_) -> const Block& { return hB[decltype(t_)::value][decltype(kb_)::value]; };
    Block xs[kRT][2];
    auto load_xs = [&] {
      static_for<kRT>([&](auto t_) {
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

    layer_tan16<M, NSB, 2, kRelu>(ring, bias, g, hA, last, in_x); convert_last_tan16<M, kRelu, NSB>(hA, last); bias += NSB * 16;
    prefetch(nxt_grp);
    int l = 1;
    for (; l + 1 < a.D; l += 2) {
      if ((a.skip_mask >> (l - 1)) & 1u) { load_xs(); layer_tan16<M, NSB, NKB + 2, kRelu>(ring, bias, g, hB, last, in_xA); }
      else layer_tan16<M, NSB, NKB, kRelu>(ring, bias, g, hB, last, in_A);
      convert_last_tan16<M, kRelu, NSB>(hB, last); bias += NSB * 16;
      if ((a.skip_mask >> l) & 1u) { load_xs(); layer_tan16<M, NSB, NKB + 2, kRelu>(ring, bias, g, hA, last, in_xB); }
      else layer_tan16<M, NSB, NKB, kRelu>(ring, bias, g, hA, last, in_B);
      convert_last_tan16<M, kRelu, NSB>(hA, last); bias += NSB * 16;
    }
    if (l < a.D) {
      if ((a.skip_mask >> (l - 1)) & 1u) { load_xs(); layer_tan16<M, NSB, NKB + 2, kRelu>(ring, bias, g, hB, last, in_xA); }
      else layer_tan16<M, NSB, NKB, kRelu>(ring, bias, g, hB, last, in_A);
      convert_last_tan16<M, kRelu, NSB>(hB, last); bias += NSB * 16;
      static_for<kRT>([&](auto t_) { static_for<NKB>([&](auto b_) { hA[decltype(t_)::value][decltype(b_)::value] = hB[decltype(t_)::value][decltype(b_)::value]; }); });
    }
    // views o feature on cat[h, dirs27] (tangent: [dh, 0]) with alpha_linear as row 0 of the last sub-block; then rgb
    Block vs[kRT];
    static_for<kRT>([&](auto t_) {
      constexpr int t = decltype(t_)::value;
      if constexpr (t < kTiles) vs[t] = stash_get(t, 2);
      else vs[t].v = typename M::AFrag{};
    });
    auto in_Av = [&](auto t_, auto kb_) -> const Block& {
      constexpr int kb = decltype(kb_)::value;
      if constexpr (kb < NKB) return hA[decltype(t_)::value][kb]; else return vs[decltype(t_)::value];
    };
    layer_tan16<M, NSB / 2 + 1, NKB + 1, kRelu>(ring, bias, g, hB, last, in_Av); bias += (NSB / 2 + 1) * 16;
    float sigma[kRT];
    static_for<kRT>([&](auto t_) { sigma[decltype(t_)::value] = last[decltype(t_)::value][0]; });
    layer_tan16<M, 1, NKB / 2, kNone>(ring, bias, g, hA, last, in_B);

    const int le = nsepi::opaque_lane();
    if (le < 16) {
      static_for<kTiles>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        const int i = (wave * kTiles + t) * 16 + le;
        nsepi::v4f o4{last[t][0], last[t][1], last[t][2], sigma[t]};
        if ((bad >> t) & 1u) { const float q = __builtin_nanf(""); o4 = nsepi::v4f{q, q, q, q}; }
        *rec.raw(i) = o4;
        *tr.draw(i) = nsepi::v4f{last[kTiles + t][0], last[kTiles + t][1], last[kTiles + t][2], sigma[kTiles + t]};
      });
    }
    nsepi::composite_group(a, rec, true, grp, gi, par, wave, le);   // the forward's outputs (barrier inside)

    // the tangents: wave 0 walks the group's rays, one lane per ray (every wave's records are in LDS: composite_group's barrier)
    if (wave == 0) {
      const int64_t s0 = grp * kGS;
      if (a.m_chunks) {
        // N = 64 m >= 128 >= kGS: the group holds the end of the ray it began in (or the whole of it) and, past that, the start
        // of the next ray, which stays open
        if (le == 0) {
          const int x0 = (gi * kGS) % a.N;                // the group's first sample, as a position in its ray
          const int n1 = a.N - x0 < kGS ? a.N - x0 : kGS;
          Walk W;
          if (x0 > 0) W.load(tr);
          walk_samples(W, rec, tr, par, 0, n1);
          if (x0 + n1 == a.N) {
            if (s0 < S_) write_jacobian(a, s0 / a.N, W);
            if (n1 < kGS) {
              Walk W2;
              walk_samples(W2, rec, tr, par, n1, kGS - n1);
              W2.store(tr);
            }
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

int tan16_program_slabs(int W, int D, uint32_t skip_mask) {   // with view directions (ob16_program_slabs, ns_nerf_mlp_ob16.hip)
  const int NSB = W / 16, NKB = W / 32, dp = kOb16Depth;
  int n = ob16_layer_slabs(NSB, 2, dp);
  for (int l = 1; l < D; ++l) n += ob16_layer_slabs(NSB, ((skip_mask >> (l - 1)) & 1u) ? NKB + 2 : NKB, dp);
  return n + ob16_layer_slabs(NSB / 2 + 1, NKB + 1, dp) + ob16_layer_slabs(1, NKB / 2, dp);
}

template <class M>
size_t tan16_lds_bytes(int bias_floats) {
  return static_cast<size_t>(PipeOf<M>::kLdsBytes) + ((static_cast<size_t>(bias_floats) * 4 + 15) & ~size_t(15)) +
         static_cast<size_t>(kWaves) * kRT * 3 * 1024 + static_cast<size_t>(kWaves) * 11 * 256 + Rec::kBytes +
         TanRecords::kBytes;
}

template <class M, int NKB>
int launch_tan16(Tan16Args& a, hipStream_t stream) {
  const size_t lds = tan16_lds_bytes<M>(a.bias_floats);
  if (lds > 160 * 1024) {
    ns::set_error("ns_render_rays_fused_tangent: %zu bytes of LDS needed (too deep a network for the resident bias image)", lds);
    return NS_E_UNSUPPORTED;
  }
  auto kern = nerf_tan16_kernel<M, NKB>;
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

// called by ns_render_rays_fused_tangent (ns_render.cpp) for an f16 handle, which it has checked
// (ns_render_tangent_supported) with the outputs: rays (o, d, view), the DepthNet depth of every ray in comp->mean_dev, the
// forward's per-ray outputs in comp
int ns_nerf_forward_ob16_tangent(const ns_weights* net, const float* o_dev, const float* d_dev, const float* viewdirs_dev,
                                 int64_t R, int N, const ns_composite_args* comp, float* d_rgb, float* d_disp, float* d_depth,
                                 float* d_acc, hipStream_t stream) {
  if (tan16_program_slabs(net->width, net->depth, net->skip_mask) != static_cast<int>(net->n_slabs)) {
    ns::set_error("ns_render_rays_fused_tangent: packed stream has %u slabs, kernel program expects %d", net->n_slabs,
                  tan16_program_slabs(net->width, net->depth, net->skip_mask));
    return NS_E_INVALID;
  }
  Tan16Args a{};
  a.stream = static_cast<const char*>(net->stream_dev);
  a.bias = net->bias_dev; a.n_slabs = net->n_slabs; a.bias_floats = net->bias_floats;
  a.D = net->depth; a.skip_mask = net->skip_mask;
  a.o = o_dev; a.d = d_dev; a.viewdirs = viewdirs_dev;
  a.S = R * N; a.N = N;
  nsepi::set_comp_args(a, comp, N);
  a.d_rgb = d_rgb; a.d_disp = d_disp; a.d_depth = d_depth; a.d_acc = d_acc;
  // (only f16 is instantiated: bf16 fields are refused)
  if (net->dtype == NS_DTYPE_F16)
    return net->width == 256 ? launch_tan16<Mma16F16, 8>(a, stream) : launch_tan16<Mma16F16, 4>(a, stream);
  ns::set_error("ns_render_rays_fused_tangent: an f16 handle is required here (dtype %d)", net->dtype);
  return NS_E_UNSUPPORTED;
}
