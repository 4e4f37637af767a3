// In-kernel sample placement and compositing of the radiance-field MLP kernels on the 16x16x32 engine (the one-kernel renderer):
// the 16-bit kernel (ns_nerf_mlp_ob16.hip, T = 4 / 5 tiles per wave) and the split-fp16 kernel (ns_nerf_mlp_x3.hip, T = 2) run
// this code with their own group shape.  A group is NWAVES x T tiles of 16 samples = T chunks of 64 consecutive samples; wave w
// holds samples w * 16 T .. (w + 1) * 16 T - 1 of it, so with T != 4 a chunk straddles waves.
//
// Args (Nerf16Args, NerfX3CompArgs, nstan::TanArgs) inherits nsepi::CompFields.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ns_composite_ray.h"
#include "ns_guard.h"
#include "ns_mlp_engine.h"
#include "ns_place.h"
#include "ns_weights.h"

namespace nsepi {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef v4f __attribute__((address_space(3))) * CrawPtr;
typedef v2f __attribute__((address_space(3))) * CzdPtr;
typedef float __attribute__((address_space(3))) * CsigPtr;
typedef uint32_t __attribute__((address_space(3))) * CslotPtr;

// The compositing fields of a kernel's argument struct (Nerf16Args, NerfX3CompArgs, nstan::TanArgs inherit them), which place_wave /
// composite_group / set_comp_args read by name.
// In-kernel compositing (the DepthNet branch of render_rays_test as ONE kernel, nerf_utils.py:836-865): comp != 0 runs
// raw2outputs (sampling_trainer.py:153-230) on the wave scan of ns_composite_ray.h in the epilogue -- raw then never
// leaves the CU (raw may be NULL).  comp == 1: depths from the array z [S];  comp == 2: sample_points_around_mean
// ("uniform", utils.py:231-241) evaluated in-kernel from the DepthNet depth mean [R] -- no z array exists.
// N is a power of two <= 64 (whole rays per 64-sample chunk) or a multiple of 64 up to 512 (whole chunks per ray).
struct CompFields {
  int comp;
  int n_shift;             // log2 N when N is a power of two, else -1
  const float* mean;
  float std_, lin_step;    // the grid linspace(-std, std, N - 1) and its step (correctly rounded on the host)
  int white_bkgd;
  float* rgb; int64_t rgb_stride;
  float* disp; int64_t disp_stride;
  float* weights;          // [S] or NULL
  float* z_out;            // [S] or NULL (comp == 2: the depths the kernel placed)
  float* pts_out;          // [S,3] or NULL
  const float* sig_last;   // NULL, or [R,4]: element 3 of row r replaces sigma of ray r's last sample (the guard pass)
  // rays longer than a 64-sample chunk (N = 64 m, m = m_chunks >= 2; 0 otherwise): a workgroup then walks sg_groups CONSECUTIVE
  // groups -- lcm(group samples, N) samples, whole rays -- before it jumps, so that a ray's chunks meet in one workgroup and
  // the transmittance / sums of the ray that is open at a group boundary carry over in LDS
  int m_chunks, sg_groups;
  // the selective guard: a ray whose own sigma of the last sample is within fix_thr of zero leaves a record at slot
  // atomicAdd(fix_count) of fix_rec (ns_guard.h: nsfix::kFloats floats for a ray of one chunk, kLongFloats for one of several)
  float fix_thr;
  uint32_t* fix_count;
  float* fix_rec;
  // the max-weight sample of every ray (nerf_utils.py:813-819), all three or none: max_z, max_w [R] and max_rgb [R,3] get the z,
  // the weight and sigmoid(raw rgb) of the sample argmax(weights) picks
  float* max_z;
  float* max_w;
  float* max_rgb;
  // the per-ray expected depth and opacity sums (ns_composite_args::depth_dev / acc_dev): [R] each, or NULL
  float* depth;
  float* acc;
};

// The lane id as a value the compiler cannot hoist: everything the compositing code derives from the lane (LDS record
// addresses per tile, the scan's lane predicates for six segment widths) would otherwise be computed ONCE before the
// group loop and kept alive across the ten layer statements -- which leave the compiler 32 VGPRs -- i.e. spilled to
// scratch and reloaded in the epilogue behind s_waitcnt vmcnt(0), waiting out the weight DMA in flight (measured: +1.5 ms
// per frame).  Two v_mbcnt per use instead.
__device__ __forceinline__ int opaque_lane() {
  uint32_t z = 0;
  asm volatile("" : "+s"(z));
  return static_cast<int>(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z)));
}

// The compositing records in LDS, from byte address `base` on (kBytes): sample i (0 .. GS - 1) of the open group
//   raw float4 per sample | {z, dist * |d|} float2 per sample, two group parities | sigma of a ray's last sample from the guard
//   pass, one float per ray of the group, two parities | 128 chunk scalars
// The chunk scalars, as float offsets:
//   kCP + c            chunk c's transmittance factor
//   kCS + 8 c + 0..4   chunk c's five sums;  + 5..7 its max-weight sample (Args::max_w != NULL): weight, z, sigmoid(raw r)
//   kOPEN + 8 p + 0..5 the open ray's {carry, r, g, b, depth, acc}, parity p;  + 6..7 its max-weight sample so far: weight, z
//   kMGB + 2 c + 0..1  chunk c's max-weight sample: sigmoid(raw g, b)
//   kMOPEN + 3 p + 0..2  the open ray's max-weight sample so far: sigmoid(raw r, g, b), parity p
//   kFIX + c           (uint32) chunk c ends a ray the selective guard flagged: 1 + the slot of its record in fix_rec; else 0
template <int T, int NWAVES>
struct Records {
  static constexpr int GS = NWAVES * T * 16;
  static constexpr uint32_t kBytes = GS * 36 + 512;
  // rays of several chunks: per chunk of the group its transmittance factor (kCP) and its five sums (kCS); the ray that is open
  // at the group's end: {carry, r, g, b, depth, acc}, two parities (kOPEN + 8 par is read, kOPEN + 8 (par ^ 1) written)
  static constexpr int kCP = 0, kCS = 8, kOPEN = 8 + 8 * 8;          // float offsets inside the 128-float scalar block
  static constexpr int kMGB = kOPEN + 16, kMOPEN = kMGB + 16, kFIX = kMOPEN + 2 * 3;
  static_assert(T <= 8, "eight chunks per group at most");
  static_assert(kFIX + 8 <= 128, "the max-weight sample's and the guard's slots end inside the 128-float scalar block (kBytes unchanged)");
  uint32_t base;
  __device__ __forceinline__ CrawPtr raw(int i) const { return reinterpret_cast<CrawPtr>(static_cast<uintptr_t>(base + static_cast<uint32_t>(i) * 16u)); }
  __device__ __forceinline__ CzdPtr zd(uint32_t par, int i) const {
    return reinterpret_cast<CzdPtr>(static_cast<uintptr_t>(base + GS * 16u + (par * GS + static_cast<uint32_t>(i)) * 8u));
  }
  __device__ __forceinline__ CsigPtr sig(uint32_t par, int ray) const {      // ray: index within the group (<= GS / 2 rays)
    return reinterpret_cast<CsigPtr>(static_cast<uintptr_t>(base + GS * 32u + (par * (GS / 2) + static_cast<uint32_t>(ray)) * 4u));
  }
  __device__ __forceinline__ CsigPtr scal(int k) const {
    return reinterpret_cast<CsigPtr>(static_cast<uintptr_t>(base + GS * 36u + static_cast<uint32_t>(k) * 4u));
  }
  __device__ __forceinline__ CslotPtr slot(int c) const {
    return reinterpret_cast<CslotPtr>(static_cast<uintptr_t>(base + GS * 36u + static_cast<uint32_t>(kFIX + c) * 4u));
  }
};

// Sample placement + the compositing record {z, dist * |d|} of every sample of the wave, ONE SAMPLE PER LANE (64 at a time: the
// tile layout holds a sample on four lanes, and a per-tile evaluation would cost T times this): sample i of the wave's 16 T on
// lane i % 64 of pass i / 64.  The records go to LDS -- the epilogue composites from them, and the caller's tiles read their
// depth back from there (same wave: LDS order suffices).
// st(slot, i): staged value `slot` of the wave's sample i -- o 0..2, d 3..5; 6: the ray's DepthNet depth (comp == 2) or the
// sample's depth (comp == 1); 10: the NEXT sample's depth (comp == 1) or the guard pass's sigma of the ray's last sample.
template <int T, int NWAVES, class Args, class Staged>
__device__ __forceinline__ void place_wave(const Args& a, const Records<T, NWAVES>& rec, Staged st, int64_t grp, int gi,
                                           uint32_t par, int wave) {
  constexpr int GS = Records<T, NWAVES>::GS;
  const int lo = opaque_lane();
  constexpr int kPasses = (16 * T + 63) / 64;
  // group-level scalars: how many of the group's GS samples exist, and the position of its first sample in its ray
  // (N <= 64 divides the group size: 0;  N = 64 m: the run starts on a ray, every group adds GS mod N)
  const int64_t left = a.S - grp * GS;
  const int rem = left < GS ? static_cast<int>(left) : GS;
  const int jg0 = a.m_chunks ? (gi * GS) % a.N : 0;                 // (wave-uniform 32-bit arithmetic, gi < 8)
#pragma unroll
  for (int pass = 0; pass < kPasses; ++pass) {
    const int i = pass * 64 + lo;
    if (i < 16 * T) {
      // every staged value of the pass in one burst, ahead of the arithmetic (slot 10 holds the next depth, the guard's
      // sigma, or nothing: read whatever is there, used only where it is defined)
      const float m_or_z = st(6, i), d0 = st(3, i), d1 = st(4, i), d2 = st(5, i), s10 = st(10, i);
      const int ig = wave * (16 * T) + i;                             // the sample's index within the group
      const bool valid = ig < rem;
      int j, ray_in_group;                                            // (a sample past the end: any in-range j, never used)
      if (!a.m_chunks) {                                              // N <= 64, a power of two: whole rays per group
        j = ig & (a.N - 1); ray_in_group = ig >> a.n_shift;
      } else {                                                        // N >= 128, jg0 + ig < GS + N <= 3.5 N
        const int x = jg0 + ig;
        ray_in_group = (x >= a.N) + (x >= 2 * a.N) + (x >= 3 * a.N);
        j = x - ray_in_group * a.N;
      }
      float zz = m_or_z, znext = s10;
      if (a.comp == 2)        // sample_points_around_mean("uniform"): depths j and j + 1 of the ray from its mean
        nsplace::uniform_z_pair(m_or_z, a.std_, a.lin_step, a.N - 1, j, zz, znext);
      const float dist_raw = (j < a.N - 1) ? znext - zz : 1e10f;      // sampling_trainer.py:176-180
      *rec.zd(par, ig) = v2f{zz, dist_raw * nscomp::ray_norm(d0, d1, d2)};
      // the guard pass's sigma of this ray's last sample: one slot per ray of the group
      if (a.sig_last && j == a.N - 1) *rec.sig(par, ray_in_group) = s10;
      if (valid && (a.z_out || a.pts_out)) {
        const int64_t sidx = grp * GS + ig;
        if (a.z_out) a.z_out[sidx] = zz;
        if (a.pts_out) {
          float* q = a.pts_out + sidx * 3;
          q[0] = st(0, i) + d0 * zz; q[1] = st(1, i) + d1 * zz; q[2] = st(2, i) + d2 * zz;
        }
      }
    }
  }
}

// The epilogue: raw2outputs (sampling_trainer.py:153-230) of the group whose raw records rec.raw() every wave has written (lane
// le < 16 of tile t of wave w: sample (w T + t) 16 + le), with the {z, dist} records of parity `par` from place_wave.  Every wave
// of the workgroup calls it (s_barrier inside unless T == 4); `comp` is a.comp != 0.
template <int T, int NWAVES, class Args>
__device__ __forceinline__ void composite_group(const Args& a, const Records<T, NWAVES>& rec, bool comp, int64_t grp, int gi,
                                                uint32_t par, int wave, int le) {
  constexpr int GS = Records<T, NWAVES>::GS;
  constexpr int kCP = Records<T, NWAVES>::kCP, kCS = Records<T, NWAVES>::kCS, kOPEN = Records<T, NWAVES>::kOPEN;
  constexpr int kMGB = Records<T, NWAVES>::kMGB, kMOPEN = Records<T, NWAVES>::kMOPEN;
  const bool afix = a.fix_rec != nullptr;   // the selective guard (wave-uniform: a kernel argument)
  const bool amax = a.max_w != nullptr;   // the max-weight sample of every ray (wave-uniform: a kernel argument)
  if (comp && a.m_chunks) {
    // Rays of m = N / 64 chunks (N = 128, 192, ...): a ray's chunks sit on different waves, possibly in different groups
    // of the workgroup's run.  Three phases around two s_barriers, the arithmetic of raw2outputs_kernel's multi-chunk
    // loop (ns_composite_ray.h: chunk_local, then T = carry * excl with the carry multiplied up chunk by chunk, every
    // chunk's sums reduced on their own and added in chunk order):
    //   1  every chunk on its wave: alpha, colours, the chunk's own transmittance scan; its factor P_c -> LDS
    //   2  carry entering the chunk = (the open ray's carry, if the ray began in an earlier group) x P of the ray's
    //      earlier chunks of this group, in order; weights; the chunk's five sums -> LDS
    //   3  lane c of the last wave, for the chunk c that ends a ray or the group: totals in chunk order; a finished ray is written,
    //      the ray that stays open hands {carry, sums} to the next group
    const int m = a.m_chunks;
    const int64_t C0 = grp * T;                      // global index of the group's first chunk
    constexpr int NCW = (T + NWAVES - 1) / NWAVES;   // chunks a wave may own
    nscomp::ChunkLocal L[NCW];
    float zc[NCW];
    bool okc[NCW];
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // every wave's raw records are in LDS
    nsmlp::static_for<NCW>([&](auto ci_) {
      constexpr int ci = decltype(ci_)::value;
      const int c = wave + NWAVES * ci;
      if (c < T) {                                   // (wave-uniform)
        const int i = c * 64 + le;
        const int64_t s_ = grp * GS + i;
        okc[ci] = s_ < a.S;
        const v4f qv = *rec.raw(i);
        const v2f zd = *rec.zd(par, i);
        float4 q = make_float4(qv.x, qv.y, qv.z, qv.w);
        if (a.sig_last) {                            // the guard pass's sigma for the ray's last sample
          const int x = (gi * GS) % a.N + i;         // position counted from the start of the group's first ray
          const int k = (x >= a.N) + (x >= 2 * a.N) + (x >= 3 * a.N);
          if (x - k * a.N == a.N - 1) q.w = *rec.sig(par, k);
        }
        L[ci] = nscomp::chunk_local<64>(okc[ci], le, q, zd.y, 1.0f, 0.0f, false);
        zc[ci] = zd.x;
        if (le == 63) *rec.scal(kCP + c) = L[ci].p;
      }
    });
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    nsmlp::static_for<NCW>([&](auto ci_) {
      constexpr int ci = decltype(ci_)::value;
      const int c = wave + NWAVES * ci;
      if (c < T) {
        const int pos = static_cast<int>((C0 + c) % m);          // the chunk's position in its ray
        const int first = c - pos;                               // the ray's first chunk, as an index of this group
        float carry = first < 0 ? *rec.scal(kOPEN + 8 * par) : 1.0f;
        for (int cc = first < 0 ? 0 : first; cc < c; ++cc) carry = carry * *rec.scal(kCP + cc);
        const float Tr = carry * L[ci].excl;
        const float w = L[ci].alpha * Tr;
        const int64_t s_ = grp * GS + c * 64 + le;
        if (okc[ci] && a.weights) a.weights[s_] = w;
        auto shares = [&]() {                                     // the lane's share of the chunk's five sums
          nscomp::RayAccum X;
          if (okc[ci]) {
            X.r += w * L[ci].cr; X.g += w * L[ci].cg; X.b += w * L[ci].cb;
            X.depth += w * zc[ci];
            X.acc += w;
          }
          return X;
        };
        nscomp::RayAccum A = shares();
        nscomp::reduce_sums<64>(A, le);
        if (le == 63) {
          *rec.scal(kCS + 8 * c + 0) = A.r; *rec.scal(kCS + 8 * c + 1) = A.g; *rec.scal(kCS + 8 * c + 2) = A.b;
          *rec.scal(kCS + 8 * c + 3) = A.depth; *rec.scal(kCS + 8 * c + 4) = A.acc;
        }
        if (__builtin_expect(afix && pos == m - 1, 0)) {
          // The selective guard, on the chunk that ends a ray (wave-uniform): lane 63 holds the ray's last sample.  A sigma within
          // fix_thr of zero (a NaN compares false: a NaN ray stays NaN) flags the ray: the wave writes the record's operands
          // (ns_guard.h) at the slot lane 63 draws, and phase 3 adds the earlier chunks' totals through kFIX.
          const int i = c * 64 + le;
          const v4f qv = *rec.raw(i);                             // (this group's until the barrier below)
          const bool flag = le == 63 && okc[ci] && __builtin_fabsf(qv.w) < a.fix_thr;
          if (le == 63 && !flag) *rec.slot(c) = 0u;
          if (__builtin_amdgcn_ballot_w64(flag)) {
            uint32_t slot = 0;
            if (le == 63) slot = atomicAdd(a.fix_count, 1u);
            slot = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(slot), 63));
            float* q = a.fix_rec + static_cast<size_t>(slot) * nsfix::kLongFloats;
            if (le == 63) {
              const v2f zd = *rec.zd(par, i);
              const int64_t r = (C0 + c) / m;
              *rec.slot(c) = slot + 1u;
              q[nsfix::kLongT] = Tr; q[nsfix::kLongRaw] = qv.x; q[nsfix::kLongRaw + 1] = qv.y;   // (kLongSum + 0 .. 4 are phase 3's)
              *reinterpret_cast<float4*>(q + nsfix::kLongRaw + 2) = make_float4(qv.z, zd.x, zd.y, nsfix::fix_ray_lo(r));
              q[nsfix::kLongRayHi] = nsfix::fix_ray_hi(r);
            }
            // x62, then u2 .. u6: lane 63 - SW after the first log2 SW steps of the 64-lane reduction, which are reduce5<SW>'s own
            nsmlp::static_for<6>([&](auto k_) {
              constexpr int k = decltype(k_)::value;
              constexpr int SW = 1 << k;
              nscomp::RayAccum X = shares();
              if constexpr (k > 0) nscomp::reduce_sums<SW>(X, le);
              if (le == (k == 0 ? 62 : 63 - SW)) {
                float* u = q + nsfix::kLongOps + nsfix::kSums * k;
                u[0] = X.r; u[1] = X.g; u[2] = X.b; u[3] = X.depth; u[4] = X.acc;
              }
            });
          }
        }
        if (__builtin_expect(amax, 0)) {   // the chunk's max-weight sample (a ray's chunks are combined in order in phase 3)
          float best = w;
          int bi = okc[ci] ? le : nscomp::kNoSample;
          nscomp::argmax_segment(best, bi, 64);
          if (bi == le) {   // its own lane records it (the raw record is this group's until the barrier below)
            const v4f qv = *rec.raw(c * 64 + le);
            *rec.scal(kCS + 8 * c + 5) = w; *rec.scal(kCS + 8 * c + 6) = zc[ci];
            *rec.scal(kCS + 8 * c + 7) = nscomp::sigmoid_ieee(qv.x);
            *rec.scal(kMGB + 2 * c) = nscomp::sigmoid_ieee(qv.y); *rec.scal(kMGB + 2 * c + 1) = nscomp::sigmoid_ieee(qv.z);
          }
        }
      }
    });
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (wave == NWAVES - 1 && le < T) {       // (the last wave: with five tiles wave 0 has had two chunks in phases 1 and 2, this one one)
      const int c = le;
      const int pos = static_cast<int>((C0 + c) % m);
      const bool ends = pos == m - 1;
      if (ends || c == T - 1) {
        const int first = c - pos;
        nscomp::RayAccum tot;                        // tot.carry: the transmittance behind chunk c
        if (first < 0) {
          tot.carry = *rec.scal(kOPEN + 8 * par); tot.r = *rec.scal(kOPEN + 8 * par + 1); tot.g = *rec.scal(kOPEN + 8 * par + 2);
          tot.b = *rec.scal(kOPEN + 8 * par + 3); tot.depth = *rec.scal(kOPEN + 8 * par + 4); tot.acc = *rec.scal(kOPEN + 8 * par + 5);
        }
        auto add_chunk = [&](int cc) {
          tot.carry = tot.carry * *rec.scal(kCP + cc);
          tot.r = tot.r + *rec.scal(kCS + 8 * cc); tot.g = tot.g + *rec.scal(kCS + 8 * cc + 1); tot.b = tot.b + *rec.scal(kCS + 8 * cc + 2);
          tot.depth = tot.depth + *rec.scal(kCS + 8 * cc + 3); tot.acc = tot.acc + *rec.scal(kCS + 8 * cc + 4);
        };
        for (int cc = first < 0 ? 0 : first; cc < c; ++cc) add_chunk(cc);
        if (__builtin_expect(afix && ends, 0)) {     // a flagged ray: its totals before the last chunk, for the fix-up
          const uint32_t slot = *rec.slot(c);
          if (slot) {
            float* q = a.fix_rec + static_cast<size_t>(slot - 1u) * nsfix::kLongFloats;
            *reinterpret_cast<float4*>(q + nsfix::kLongSum) = make_float4(tot.r, tot.g, tot.b, tot.depth);
            q[nsfix::kLongSum + 4] = tot.acc;
          }
        }
        add_chunk(c);
        // the ray's max-weight sample: the open ray's so far, then its chunks of this group in order (a later chunk's samples
        // have larger indices: it wins only where nscomp::beats says so without the index -- a larger weight, or the first NaN)
        float mw = 0.0f, mz = 0.0f, mr = 0.0f, mg = 0.0f, mb = 0.0f;
        if (__builtin_expect(amax, 0)) {
          if (first < 0) {
            mw = *rec.scal(kOPEN + 8 * par + 6); mz = *rec.scal(kOPEN + 8 * par + 7);
            mr = *rec.scal(kMOPEN + 3 * par); mg = *rec.scal(kMOPEN + 3 * par + 1); mb = *rec.scal(kMOPEN + 3 * par + 2);
          }
          for (int cc = first < 0 ? 0 : first; cc <= c; ++cc) {
            const float v = *rec.scal(kCS + 8 * cc + 5);
            if (cc == first || (v != v ? mw == mw : v > mw)) {
              mw = v; mz = *rec.scal(kCS + 8 * cc + 6); mr = *rec.scal(kCS + 8 * cc + 7);
              mg = *rec.scal(kMGB + 2 * cc); mb = *rec.scal(kMGB + 2 * cc + 1);
            }
          }
        }
        if (ends) {
          const int64_t r = (C0 + c) / m;
          if (r * a.N < a.S) {
            float disp;
            nscomp::finish_totals(tot, a.white_bkgd, disp);
            float* prgb = a.rgb + r * a.rgb_stride;
            prgb[0] = tot.r; prgb[1] = tot.g; prgb[2] = tot.b;
            a.disp[r * a.disp_stride] = disp;
            if (a.depth) a.depth[r] = tot.depth;      // (wave-uniform tests: kernel arguments)
            if (a.acc) a.acc[r] = tot.acc;            // (finish_totals adds the white background to rgb only)
            if (amax) {
              a.max_w[r] = mw; a.max_z[r] = mz;
              a.max_rgb[r * 3] = mr; a.max_rgb[r * 3 + 1] = mg; a.max_rgb[r * 3 + 2] = mb;
            }
          }
        } else {                                     // the ray goes on in the workgroup's next group
          const uint32_t np = par ^ 1u;
          *rec.scal(kOPEN + 8 * np) = tot.carry; *rec.scal(kOPEN + 8 * np + 1) = tot.r; *rec.scal(kOPEN + 8 * np + 2) = tot.g;
          *rec.scal(kOPEN + 8 * np + 3) = tot.b; *rec.scal(kOPEN + 8 * np + 4) = tot.depth; *rec.scal(kOPEN + 8 * np + 5) = tot.acc;
          if (amax) {
            *rec.scal(kOPEN + 8 * np + 6) = mw; *rec.scal(kOPEN + 8 * np + 7) = mz;
            *rec.scal(kMOPEN + 3 * np) = mr; *rec.scal(kMOPEN + 3 * np + 1) = mg; *rec.scal(kMOPEN + 3 * np + 2) = mb;
          }
        }
      }
    }
  } else if (comp) {
    // raw2outputs in the epilogue (sampling_trainer.py:153-230): the group's samples are T chunks of 64 consecutive
    // samples -- whole rays (N <= 64, a power of two) -- one chunk per wave pass, composited by the lane-level code the
    // stand-alone kernel runs (ns_composite_ray.h: same operations in the same order, so bit-identical to it).
    // Four tiles: a wave's chunk is its own 64 samples, the wave's own LDS order suffices; two or five tiles: chunks straddle
    // waves, one s_barrier (all four waves reach it: the group loop is workgroup-uniform).
    if constexpr (T == 4) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // (amax) the lane's sample for the ray's argmax below the switch -- one copy of that code for the six segment widths: its
    // weight, its index in the ray (kNoSample past the end), depth and raw
    float mx_w = 0.0f, mx_z = 0.0f;
    int mx_i = nscomp::kNoSample;
    float4 mx_q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    auto composite = [&](auto sw_, int c) {
      constexpr int SW = decltype(sw_)::value;
      const int i = c * 64 + le;
      const int64_t s = grp * GS + i;
      const bool ok = s < a.S;
      const v4f qv = *rec.raw(i);
      const v2f zd = *rec.zd(par, i);
      float4 q = make_float4(qv.x, qv.y, qv.z, qv.w);
      if (a.sig_last && (le & (SW - 1)) == SW - 1) q.w = *rec.sig(par, i / SW);      // the guard pass's sigma_last
      nscomp::RayAccum A, tree;
      float alpha, w, disp, Tr;
      const int sub = le & (SW - 1);
      nscomp::composite_chunk<SW>(A, ok, sub, q, zd.x, zd.y, 1.0f, 0.0f, false, alpha, w, &Tr);
      if (ok && a.weights) a.weights[s] = w;
      if (__builtin_expect(amax, 0)) { mx_w = w; mx_i = ok ? sub : nscomp::kNoSample; mx_z = zd.x; mx_q = q; }
      nscomp::composite_finish<SW>(A, a.white_bkgd, disp, sub, &tree);
      if (ok && sub == SW - 1) {
        const int64_t r = s / SW;      // N == SW
        float* prgb = a.rgb + r * a.rgb_stride;
        prgb[0] = A.r; prgb[1] = A.g; prgb[2] = A.b;
        a.disp[r * a.disp_stride] = disp;
        if (a.depth) a.depth[r] = A.depth;
        if (a.acc) a.acc[r] = A.acc;
        if (a.fix_rec && __builtin_fabsf(q.w) < a.fix_thr) {      // (a NaN sigma compares false: a NaN ray stays NaN)
          float* fr = a.fix_rec + static_cast<size_t>(atomicAdd(a.fix_count, 1u)) * nsfix::kFloats;
          *reinterpret_cast<float4*>(fr + nsfix::kSum) = make_float4(tree.r, tree.g, tree.b, tree.depth);
          *reinterpret_cast<float4*>(fr + nsfix::kSum + 4) = make_float4(tree.acc, Tr, q.x, q.y);
          *reinterpret_cast<float4*>(fr + nsfix::kRaw + 2) = make_float4(q.z, zd.x, zd.y, nsfix::fix_ray_lo(r));
          fr[nsfix::kRayHi] = nsfix::fix_ray_hi(r);
        }
      }
    };
    for (int c = wave; c < T; c += NWAVES) {
      switch (a.N) {
        case 64: composite(std::integral_constant<int, 64>{}, c); break;
        case 32: composite(std::integral_constant<int, 32>{}, c); break;
        case 16: composite(std::integral_constant<int, 16>{}, c); break;
        case 8: composite(std::integral_constant<int, 8>{}, c); break;
        case 4: composite(std::integral_constant<int, 4>{}, c); break;
        default: composite(std::integral_constant<int, 2>{}, c); break;
      }
      if (__builtin_expect(amax, 0)) {     // the ray's max-weight sample over its N-lane segment; its own lane writes it
        float best = mx_w;
        int bi = mx_i;
        nscomp::argmax_segment(best, bi, a.N);
        if (mx_i != nscomp::kNoSample && bi == mx_i) {   // (a segment past the end has no sample: nothing is written)
          const int64_t r = (grp * GS + c * 64 + le) / a.N;
          a.max_w[r] = mx_w; a.max_z[r] = mx_z;
          float* prgb = a.max_rgb + r * 3;
          prgb[0] = nscomp::sigmoid_ieee(mx_q.x); prgb[1] = nscomp::sigmoid_ieee(mx_q.y); prgb[2] = nscomp::sigmoid_ieee(mx_q.z);
        }
      }
    }
  }
}

// The host side: the compositing fields of Args from the renderer's ns_composite_args (the selective guard's fields are the
// caller's); sg_groups is set at launch, from the kernel's group size
template <class Args>
inline void set_comp_args(Args& a, const ns_composite_args* comp, int N) {
  a.comp = comp->mean_dev ? 2 : 1;
  a.mean = comp->mean_dev; a.std_ = comp->std_; a.lin_step = nsplace::linspace_step_of(-comp->std_, comp->std_, N - 1);
  a.n_shift = -1;
  for (int k = 0; k < 31; ++k) if (N == (1 << k)) a.n_shift = k;
  a.m_chunks = N > 64 ? N / 64 : 0;
  a.white_bkgd = comp->white_bkgd;
  a.rgb = comp->rgb_dev; a.rgb_stride = comp->rgb_stride; a.disp = comp->disp_dev; a.disp_stride = comp->disp_stride;
  a.weights = comp->weights_dev; a.z_out = comp->z_out_dev; a.pts_out = comp->pts_out_dev;
  a.sig_last = comp->sigma_last_dev;
  a.max_z = comp->max_z_dev; a.max_w = comp->max_w_dev; a.max_rgb = comp->max_rgb_dev;
  a.depth = comp->depth_dev; a.acc = comp->acc_dev;
}
// runs of lcm(group samples, N) / group samples consecutive groups (whole rays per run) when rays span several chunks, else 1
inline int run_groups(int group_samples, int m_chunks, int N) {
  if (!m_chunks) return 1;
  int x = group_samples, y = N;
  while (y) { const int t = x % y; x = y; y = t; }
  return N / x;   // lcm(gs, N) / gs
}

}  // namespace nsepi
