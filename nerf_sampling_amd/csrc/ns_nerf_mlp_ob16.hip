// Radiance-field MLP forward for the 16-bit operand paths (bf16 / f16) on v_mfma_f32_16x16x32: the shape that
// sustains the most under the MI355X power cap (tools/mfma_peak.hip: 2.14 vs 1.87 PFLOP/s for 32x32x16 with live
// operands).  Same operator as ns_nerf_mlp.hip (run_network + NeRF.forward, Trainer.py:789-806 and
// run_nerf_helpers.py:67-134): positional encoding of points and view directions, DxW trunk with the input skip,
// (feature o view) layer carrying the sigma head as one extra output row, rgb head, one persistent kernel.  A wave owns T = 4 tiles of 16 samples (64 samples);
// every A fragment (16 output rows x 32 input features, 1 KiB) read from LDS feeds 4 MFMAs; layers are walked one
// 16-row output sub-block at a time (layer_ob16 in ns_mlp_engine.h; weight stream layout 16 of ns_pack.hip).
#include "ns_common.h"
#include "ns_comp_epilogue.h"
#include "ns_mlp_engine.h"
#include "ns_weights.h"

// This file is compiled five times: as itself; with -DNS_OB16_TU_T5 as a second translation unit that holds only the
// five-tile production kernels; with -DNS_OB16_TU_RENDER as a third that holds only the five-tile RENDER kernels,
// nerf_render_ob16_kernel; with -DNS_OB16_TU_RENDER -DNS_OB16_TU_KBSKIP as a fourth that holds only the K-BLOCK-SKIPPING
// render kernels, nerf_kbskip_ob16_kernel; and with -DNS_OB16_TU_RENDER -DNS_OB16_TU_KSUFFIX as a fifth that holds only the
// DEAD-SUFFIX render kernels, nerf_ksuffix_ob16_kernel (the units build in parallel; each is minutes of register allocation).
//
// The render kernel is the five-tile production kernel on the sigma-first weight stream (ns_weights::stream2_dev: same chunks,
// the tail re-ordered to sigma sub-block | eight colour sub-blocks | rgb head), for launches that composite in the kernel and
// hand out nothing that reads raw rgb of a zero-weight sample (render_eligible below).  After the sigma statement every wave
// decides alone whether its 80 samples can contribute; if none can it runs the DRAIN twins of the colour and the rgb
// statement (tools/gen_ob16_asm.py --render: the same slabs, vmcnt waits, barriers, refill pieces and read-ahead, no MFMA), so
// the four waves of the workgroup keep walking the one weight ring in step with no vote and no extra barrier.
// Why the results are bit-identical to the production kernel's.  A wave skips only if every one of its samples has
// sigma <= 0 (a NaN compares false; the comparison is IEEE's, so a -0 would count -- the sigma sub-block's zero-padded view
// K-block adds +0 products, so the accumulator never is -0), none is flagged `bad` and every {z, dist |d|} record is finite.  Then
// relu(sigma) * dist = +-0, v_exp_f32(+-0) = 1 exactly, alpha = 1 - 1 = +0 and the weight w = +0 * T = +0 (T >= 0; a NaN T stays
// NaN whatever the colour is).  The skipping wave writes (0, 0, 0, sigma) records: the colour enters every sum of raw2outputs
// as w * sigmoid(raw) = +0 * sigmoid(0) = +0 = +0 * sigmoid(the real raw), for every finite real raw -- and raw is finite
// whenever the weights are and no activation overflows the operand type (fp16: 65504).  KNOWN DIVERGENCE, not enforced: an
// overflow in the trunk reaches sigma too (inf * w = inf or NaN: the wave does not skip), but an fp16 field whose view-layer
// activations alone overflow to inf gives NaN rgb on the production kernel (inf * 0 in the rgb head) and 0 here, for samples of
// zero weight.  It cannot be seen without computing the colour layers; ns_debug_set("no_colour_skip", 1) is the way out.  Outputs that read raw rgb without the weight (raw itself, the
// max-weight sample, the guards' records) keep a launch on the production kernel.
//
// The K-block-skipping render kernel (NS_OB16_TU_KBSKIP) is the render kernel with trunk layers 3..7, sigma and colour from
// ns_ob16_kbskip_asm.inc (tools/gen_ob16_asm.py --kbskip).  Layers 3..7 also return a live mask of their tested output K-blocks
// (32 hidden units x the wave's 80 samples; a bit is 0 iff every packed 16-bit activation of the block is the bit pattern 0x0000),
// and the statement that consumes the block branches around the five MFMAs of each chunk step that would multiply it.
// Why the results are bit-identical to the render kernel's on the same handle.  (1) Samples are the columns of every MFMA: a dead
// K-block is dead for all 80 columns of the wave, so no sample's sum loses a term that another wave's decision made.  (2) The
// products of a skipped step are w * (+0) with w finite (ns_pack.hip refuses the kernel to a handle with an inf / NaN weight:
// ns_weights::kbskip_ok), so every one of them is +0 or -0 and so is their sum; acc + (+-0) == acc bit for bit unless acc is
// a zero of the other sign.  (3) That last case cannot reach an output: every skipped sum feeds either a hidden layer's packed
// ReLU -- v_cvt_pk turns +-0 into 0x0000 / 0x8000 and v_pk_max_i16(x, 0) turns both into 0x0000 -- or sigma, which this kernel's
// launches only use as `sigma <= 0` (the colour skip; true for both zeros) and as relu(sigma) * dist -> exp(-(+-0)) = 1,
// alpha = +0: no eligible launch hands raw out (render_eligible).  (4) A sub-block's first step is never skipped, so the bias
// always enters; a NaN or an inf ACTIVATION has non-zero bits and keeps its K-block live, and so would a -0 (0x8000) had the
// ReLU let one through.  (5) The test is on the bits the MFMAs would read, after the ReLU, not on values recomputed elsewhere.
// The matrix cores are taken to add a sum of zeros to a subnormal accumulator without flushing it, as they do on gfx942 / gfx950.
// OFF by default: ns_debug_set("kblock_skip", 1) (or NS_KBLOCK_SKIP=1) sends the render kernel's launches here.  On the bench frame
// the kernel skips 12.8 % of its chunk steps and is no faster than the render kernel on the same handle: a skipped step still
// issues its seven gap instructions, and the mask ORs, tests and branches cost what the skipped MFMAs save.
//
// The dead-suffix render kernel (NS_OB16_TU_KSUFFIX) is the K-block-skipping kernel with the statements of
// ns_ob16_ksuffix_asm.inc (tools/gen_ob16_asm.py --ksuffix): the same masks, but a consumer tests nothing per step -- at its start it
// takes d = the trailing dead K-blocks of its input's mask (the unit order makes dead blocks a suffix) and runs the straight-line
// body that lacks those d K-blocks' steps; a dead block above the suffix is computed.  It skips a subset of the steps the
// K-block-skipping kernel skips, so the bit-identity argument above applies unchanged.  ns_debug_set("kblock_suffix", v) /
// NS_KBLOCK_SUFFIX: 0 never, 1 every launch the render kernel takes on a kbskip_ok handle, 2 those on handles packed with the
// unit order (ns_weights_set_unit_ordered); "kblock_skip" = 1 wins over it.
namespace nsob16 {
// the field inputs, and what in-kernel placement and compositing takes (ns_comp_epilogue.h)
struct Nerf16Args : nsmlp::FieldArgs, nsepi::CompFields {
  uint32_t* skip_count;   // render kernels only: NULL, or three device counters: [0] bumped once per wave that skipped its colour
                          // statements, [1] (K-block-skipping kernel) by the chunk steps whose MFMAs a wave jumped over, [2] (dead-
                          // suffix kernel) by the chunk steps absent from the bodies a wave ran
};
// the five-tile production kernel (PROD, 80 samples per wave): defined in the NS_OB16_TU_T5 unit
int launch_prod_t5(int dtype, bool embedded, Nerf16Args& a, hipStream_t stream);
// the five-tile render kernel on the sigma-first stream (a.stream / a.bias name it): defined in the NS_OB16_TU_RENDER unit
int launch_render_t5(int dtype, Nerf16Args& a, hipStream_t stream);
// the K-block-skipping render kernel (same stream, same launches): defined in the NS_OB16_TU_KBSKIP unit
int launch_kbskip_t5(int dtype, Nerf16Args& a, hipStream_t stream);
// the dead-suffix render kernel (same stream, same launches): defined in the NS_OB16_TU_KSUFFIX unit
int launch_ksuffix_t5(int dtype, Nerf16Args& a, hipStream_t stream);
}  // namespace nsob16

#if defined(NS_OB16_TU_KBSKIP) && !defined(NS_OB16_TU_RENDER)
#error "the K-block-skipping unit is a render unit: -DNS_OB16_TU_RENDER -DNS_OB16_TU_KBSKIP"
#endif
#if defined(NS_OB16_TU_KSUFFIX) && (!defined(NS_OB16_TU_RENDER) || defined(NS_OB16_TU_KBSKIP))
#error "the dead-suffix unit is a render unit of its own: -DNS_OB16_TU_RENDER -DNS_OB16_TU_KSUFFIX"
#endif
#if defined(NS_OB16_TU_KBSKIP) || defined(NS_OB16_TU_KSUFFIX)
#define NS_OB16_TU_KMASK          // the unit's trunk layers 3..7, sigma and colour hand live masks on (kbs_*_asm_run of its .inc)
#endif
#ifdef NS_OB16_TU_KSUFFIX
#define NS_OB16_KERNEL nerf_ksuffix_ob16_kernel
#elif defined(NS_OB16_TU_KBSKIP)
#define NS_OB16_KERNEL nerf_kbskip_ob16_kernel
#elif defined(NS_OB16_TU_RENDER)
#define NS_OB16_KERNEL nerf_render_ob16_kernel
#else
#define NS_OB16_KERNEL nerf_mlp_ob16_kernel
#endif
#if !defined(NS_OB16_TU_T5) && !defined(NS_OB16_TU_RENDER)
#define NS_OB16_TU_MAIN
#endif

namespace {

using namespace nsmlp;

#ifndef NS_NERF16_T
#define NS_NERF16_T 4
#endif
#ifndef NS_NERF16_WAVES
#define NS_NERF16_WAVES 4
#endif
#ifndef NS_OB16_PROD_T
#define NS_OB16_PROD_T 0          // 16-sample tiles per wave in the production kernel: 4, 5, or 0 = chosen per launch
#endif
constexpr int kT = NS_NERF16_T;          // 16-sample tiles per wave
constexpr int kWaves = NS_NERF16_WAVES;  // 4: one wave per SIMD, ~256 AGPRs of activations + accumulators per wave
                                         // (8 waves x T = 2, two per SIMD in 256 registers each: measured slower)
// dynamic LDS (FieldLds): embedding stash per wave T x 3 blocks x 1 KiB, input staging per wave 11 rows of 16 T floats, and when
// the launch composites: raw float4 per sample of the group | {z, dist} float2 per sample, two group parities | sigma of a ray's
// last sample from the guard pass, one float per ray of the group, two parities (nsepi::Records)
template <int T>
using Ob16Lds = FieldLds<kWaves, T * 3 * 1024, 11 * (T * 64)>;

}  // namespace
#ifndef NS_OB16_ASM_INC
#define NS_OB16_ASM_INC "ns_ob16_asm.inc"
#endif
#include NS_OB16_ASM_INC
#ifdef NS_OB16_TU_RENDER
#include "ns_ob16_render_asm.inc"
#endif
#ifdef NS_OB16_TU_KBSKIP
#include "ns_ob16_kbskip_asm.inc"
#endif
#ifdef NS_OB16_TU_KSUFFIX
#include "ns_ob16_ksuffix_asm.inc"
#endif
namespace {
#ifdef NS_OB16_TU_RENDER
constexpr bool kRenderTU = true;
#else
constexpr bool kRenderTU = false;
#endif
// One W = 256 hidden layer (ReLU) as a generated asm statement: set A (hA, AGPRs) -> set V (hB, VGPRs) or back; SKIP:
// K-blocks 0, 1 are the embedded point xs.  Same chunk walk, ring protocol and arithmetic as layer_ob16<> +
// convert_last16<> (bit-identical results); the ring's bookkeeping is handed over and taken back here.
template <class M, int T, bool IN_A, bool SKIP, class PipeT>
__device__ __forceinline__ void hidden_layer_asm(PipeT& ring, const float* bias_lds, int g, typename M::Block (&hA)[T][8],
                                                 typename M::Block (&hB)[T][8], const typename M::Block (&xs)[T][2]) {
  u32x4 A[8 * T], V[8 * T], X[2 * T];
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<8>([&](auto kb_) {
      constexpr int kb = decltype(kb_)::value;
      if constexpr (IN_A) A[8 * t + kb] = __builtin_bit_cast(u32x4, hA[t][kb].v);
      else V[8 * t + kb] = __builtin_bit_cast(u32x4, hB[t][kb].v);
    });
    static_for<2>([&](auto kb_) { X[2 * t + decltype(kb_)::value] = __builtin_bit_cast(u32x4, xs[t][decltype(kb_)::value].v); });
  });
  hidden_asm_run<M, T, IN_A, SKIP>(ring, bias_lds, g, A, V, X);
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<8>([&](auto kb_) {
      constexpr int kb = decltype(kb_)::value;
      if constexpr (IN_A) hB[t][kb].v = __builtin_bit_cast(typename M::AFrag, V[8 * t + kb]);
      else hA[t][kb].v = __builtin_bit_cast(typename M::AFrag, A[8 * t + kb]);
    });
  });
}
// the other three layers of the production network as generated statements: layer 0, the view layer with
// the sigma sub-block, the rgb head
template <class M, int T, class PipeT>
__device__ __forceinline__ void layer0_asm(PipeT& ring, const float* bias_lds, int g, const typename M::Block (&xe)[T][2],
                                           typename M::Block (&hA)[T][8]) {
  u32x4 X[2 * T], A[8 * T];
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    X[2 * t] = __builtin_bit_cast(u32x4, xe[t][0].v); X[2 * t + 1] = __builtin_bit_cast(u32x4, xe[t][1].v);
  });
  layer0_asm_run<M, T>(ring, bias_lds, g, X, A);
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<8>([&](auto kb_) { hA[t][decltype(kb_)::value].v = __builtin_bit_cast(typename M::AFrag, A[8 * t + decltype(kb_)::value]); });
  });
}
template <class M, int T, class PipeT>
__device__ __forceinline__ void views_asm(PipeT& ring, const float* bias_lds, int g, const typename M::Block (&hB)[T][8],
                                          const typename M::Block (&vs)[T], typename M::Block (&hA)[T][8], f32x4a (&last)[T]) {
  u32x4 V[8 * T], D[T], A[4 * T], ACCO[T];
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<8>([&](auto kb_) { V[8 * t + decltype(kb_)::value] = __builtin_bit_cast(u32x4, hB[t][decltype(kb_)::value].v); });
    D[t] = __builtin_bit_cast(u32x4, vs[t].v);
  });
  views_asm_run<M, T>(ring, bias_lds, g, V, D, A, ACCO);
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<4>([&](auto kb_) { hA[t][decltype(kb_)::value].v = __builtin_bit_cast(typename M::AFrag, A[4 * t + decltype(kb_)::value]); });
    last[t] = __builtin_bit_cast(f32x4a, ACCO[t]);
  });
}
template <class M, int T, class PipeT>
__device__ __forceinline__ void rgb_asm(PipeT& ring, const float* bias_lds, int g, const typename M::Block (&hA)[T][8], f32x4a (&last)[T]) {
  u32x4 A[4 * T], ACCO[T];
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<4>([&](auto kb_) { A[4 * t + decltype(kb_)::value] = __builtin_bit_cast(u32x4, hA[t][decltype(kb_)::value].v); });
  });
  rgb_asm_run<M, T>(ring, bias_lds, g, A, ACCO);
  static_for<T>([&](auto t_) { last[decltype(t_)::value] = __builtin_bit_cast(f32x4a, ACCO[decltype(t_)::value]); });
}

#ifdef NS_OB16_TU_RENDER
// the sigma-first tail (ns_ob16_render_asm.inc): the view layer's sigma sub-block, its eight colour sub-blocks, the rgb head
// (sigma hands the embedded direction D on to colour in its registers; only row 0 of the sigma sub-block is kept)
template <class M, int T, class PipeT>
__device__ __forceinline__ void render_sigma_asm(PipeT& ring, const float* bias_lds, int g, const typename M::Block (&hB)[T][8],
                                                 u32x4 (&D)[T], float (&sigma)[T]) {
  u32x4 V[8 * T], ACCO[T];
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<8>([&](auto kb_) { V[8 * t + decltype(kb_)::value] = __builtin_bit_cast(u32x4, hB[t][decltype(kb_)::value].v); });
  });
  render_sigma_asm_run<M, T>(ring, bias_lds, g, V, D, ACCO);
  static_for<T>([&](auto t_) { sigma[decltype(t_)::value] = __builtin_bit_cast(f32x4a, ACCO[decltype(t_)::value])[0]; });
}
template <class M, int T, class PipeT>
__device__ __forceinline__ void render_colour_asm(PipeT& ring, const float* bias_lds, int g, const typename M::Block (&hB)[T][8],
                                                  const u32x4 (&D)[T], typename M::Block (&hA)[T][8]) {
  u32x4 V[8 * T], A[4 * T];
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<8>([&](auto kb_) { V[8 * t + decltype(kb_)::value] = __builtin_bit_cast(u32x4, hB[t][decltype(kb_)::value].v); });
  });
  render_colour_asm_run<M, T>(ring, bias_lds, g, V, D, A);
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<4>([&](auto kb_) { hA[t][decltype(kb_)::value].v = __builtin_bit_cast(typename M::AFrag, A[4 * t + decltype(kb_)::value]); });
  });
}
template <class M, int T, class PipeT>
__device__ __forceinline__ void render_rgb_asm(PipeT& ring, const float* bias_lds, int g, const typename M::Block (&hA)[T][8], f32x4a (&last)[T]) {
  u32x4 A[4 * T], ACCO[T];
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<4>([&](auto kb_) { A[4 * t + decltype(kb_)::value] = __builtin_bit_cast(u32x4, hA[t][decltype(kb_)::value].v); });
  });
  render_rgb_asm_run<M, T>(ring, bias_lds, g, A, ACCO);
  static_for<T>([&](auto t_) { last[decltype(t_)::value] = __builtin_bit_cast(f32x4a, ACCO[decltype(t_)::value]); });
}
#endif

#ifdef NS_OB16_TU_KMASK
// the statements of ns_ob16_kbskip_asm.inc / ns_ob16_ksuffix_asm.inc (five tiles): a trunk layer that returns the live mask of its output K-blocks and
// (KIND > 0) skips the steps of its input's dead ones; sigma and colour as consumers of the trunk's mask
template <class M, int KIND, bool IN_A, class PipeT>
__device__ __forceinline__ uint32_t kbs_hidden_layer_asm(PipeT& ring, const float* bias_lds, int g, typename M::Block (&hA)[5][8],
                                                         typename M::Block (&hB)[5][8], const typename M::Block (&xs)[5][2], uint32_t kmask) {
  constexpr int T = 5;
  u32x4 A[8 * T], V[8 * T], X[2 * T];
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<8>([&](auto kb_) {
      constexpr int kb = decltype(kb_)::value;
      if constexpr (IN_A) A[8 * t + kb] = __builtin_bit_cast(u32x4, hA[t][kb].v);
      else V[8 * t + kb] = __builtin_bit_cast(u32x4, hB[t][kb].v);
    });
    static_for<2>([&](auto kb_) { X[2 * t + decltype(kb_)::value] = __builtin_bit_cast(u32x4, xs[t][decltype(kb_)::value].v); });
  });
  const uint32_t omask = kbs_hidden_asm_run<M, KIND>(ring, bias_lds, g, A, V, X, kmask);
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<8>([&](auto kb_) {
      constexpr int kb = decltype(kb_)::value;
      if constexpr (IN_A) hB[t][kb].v = __builtin_bit_cast(typename M::AFrag, V[8 * t + kb]);
      else hA[t][kb].v = __builtin_bit_cast(typename M::AFrag, A[8 * t + kb]);
    });
  });
  return omask;
}
template <class M, class PipeT>
__device__ __forceinline__ void kbs_sigma_asm(PipeT& ring, const float* bias_lds, int g, const typename M::Block (&hB)[5][8], u32x4 (&D)[5],
                                              float (&sigma)[5], uint32_t kmask) {
  constexpr int T = 5;
  u32x4 V[8 * T], ACCO[T];
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<8>([&](auto kb_) { V[8 * t + decltype(kb_)::value] = __builtin_bit_cast(u32x4, hB[t][decltype(kb_)::value].v); });
  });
  kbs_sigma_asm_run<M>(ring, bias_lds, g, V, D, ACCO, kmask);
  static_for<T>([&](auto t_) { sigma[decltype(t_)::value] = __builtin_bit_cast(f32x4a, ACCO[decltype(t_)::value])[0]; });
}
template <class M, class PipeT>
__device__ __forceinline__ void kbs_colour_asm(PipeT& ring, const float* bias_lds, int g, const typename M::Block (&hB)[5][8], const u32x4 (&D)[5],
                                               typename M::Block (&hA)[5][8], uint32_t kmask) {
  constexpr int T = 5;
  u32x4 V[8 * T], A[4 * T];
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<8>([&](auto kb_) { V[8 * t + decltype(kb_)::value] = __builtin_bit_cast(u32x4, hB[t][decltype(kb_)::value].v); });
  });
  kbs_colour_asm_run<M>(ring, bias_lds, g, V, D, A, kmask);
  static_for<T>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    static_for<4>([&](auto kb_) { hA[t][decltype(kb_)::value].v = __builtin_bit_cast(typename M::AFrag, A[4 * t + decltype(kb_)::value]); });
  });
}
#endif

using nsob16::Nerf16Args;

// PROD: the production network (8 x 256, skips = [4], view directions: experiments/run.py) as straight-line code whose
// seven hidden layers are the generated asm statements -- no loop over layers, so the activation sets stay in the registers
// the statements pin them to; every other network takes the generic, compiler-scheduled path.
template <class M, int NKB, bool EMBEDDED, bool PROD = false, int TT = kT>   // NKB = W / 32 K-blocks of a hidden layer
__global__ void __launch_bounds__(kWaves * 64)
NS_OB16_KERNEL(Nerf16Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int T = TT, NWAVES = kWaves, NSB = 2 * NKB;   // 16-row output sub-blocks of a hidden layer
  using Block = typename M::Block;
  using PipeT = Pipe<M, NWAVES, kOb16Depth, kOb16Ahead>;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;

  using Lds = Ob16Lds<T>;
  constexpr uint32_t kBiasAt = Lds(0, 0).bias;
  float* bias_lds = reinterpret_cast<float*>(smem + kBiasAt);
  for (int i = threadIdx.x; i < a.bias_floats; i += NWAVES * 64) bias_lds[i] = a.bias[i];
  __syncthreads();

  const uint32_t lds0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(NS_LDS_PTR(smem)));
  const Lds lm(a.bias_floats, 0);   // (the records, when the launch asked for them, are the last region: no offset depends on them)
  typedef typename M::AFrag __attribute__((address_space(3))) * StashPtr;
  const uint32_t stash_base = lds0 + lm.stash + static_cast<uint32_t>(wave) * Lds::kWaveStash + static_cast<uint32_t>(lane) * 16u;
  auto stash_at = [&](int t, int b) -> StashPtr {
    return reinterpret_cast<StashPtr>(static_cast<uintptr_t>(stash_base + (t * 3 + b) * 1024));
  };
  auto stash_put = [&](int t, int b, const Block& v) { *stash_at(t, b) = v.v; };
  auto stash_get = [&](int t, int b) -> Block { Block v; v.v = *stash_at(t, b); return v; };
  // staging: value slot k (0..10) of sample j (0 .. 16 T - 1) of this wave's group at stage_base + k * kStageRow + j * 4
  constexpr uint32_t kStageRow = T * 64, kStageRows = 11;
  static_assert(kStageRows * kStageRow == Lds::kWaveStage, "a wave's staging rows");
  const uint32_t stage_base = lds0 + lm.stage + static_cast<uint32_t>(wave) * Lds::kWaveStage;
  // compositing records (only allocated when a.comp): ns_comp_epilogue.h
  const nsepi::Records<T, NWAVES> rec{lds0 + lm.rec};
  using nsepi::v4f;

  PipeT ring;
  ring.init(a.stream, smem, a.n_slabs, wave, lane);

  const int64_t n_tiles = (a.S + 15) / 16;
  const int64_t n_groups = (n_tiles + NWAVES * T - 1) / (NWAVES * T);
  // sample held by lane `l16` (0..15) of tile t of this wave in group grp; clamped to a real sample
  auto sample_of = [&](int64_t grp, int t, int l16, bool& valid) -> int64_t {
    const int64_t sidx = ((grp * NWAVES + wave) * T + t) * 16 + l16;
    valid = sidx < a.S;
    return valid ? sidx : a.S - 1;
  };
  // Inputs of the NEXT group are fetched right after layer 0 of the current one by LDS-DMA (no registers held across
  // the network): lane j of the wave fetches the ten values of the j-th of the wave's 64 consecutive samples.
  // pts mode: p 0..2, v 7..9;  (o, d, z) mode: o 0..2, d 3..5, z 6, v 7..9;  compositing: slot 6 is the ray's DepthNet depth
  // when the samples are placed in-kernel (comp == 2), slot 10 the NEXT sample's depth when they come from z (comp == 1).
  auto prefetch_round = [&](int64_t grp, int tile0) {     // the active lanes fetch tiles tile0 .. tile0 + 3 (clamped to T - 1)
    bool valid;
    const int tl = tile0 + (lane >> 4);
    const int64_t sidx = sample_of(grp, tl < T ? tl : T - 1, lane & 15, valid);   // (surplus lanes re-fetch, harmlessly)
    const int64_t ray = a.S <= 0x7fffffff ? static_cast<int64_t>(static_cast<uint32_t>(sidx) / static_cast<uint32_t>(a.N))
                                          : sidx / a.N;
    auto put = [&](int slot, const float* src) {
      lds_dma4(src, stage_base + slot * kStageRow + tile0 * 64);
    };
    if (a.pts) {
#pragma unroll
      for (int c = 0; c < 3; ++c) put(c, a.pts + sidx * 3 + c);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) { put(c, a.o + ray * 3 + c); put(3 + c, a.d + ray * 3 + c); }
      if (a.comp == 2) put(6, a.mean + ray);
      else put(6, a.z + sidx);
      if (a.comp == 1) put(10, a.z + (sidx + 1 < a.S ? sidx + 1 : sidx));
      else if (a.sig_last) put(10, a.sig_last + ray * 4 + 3);
    }
    if (a.use_viewdirs) {
#pragma unroll
      for (int c = 0; c < 3; ++c) put(7 + c, a.viewdirs + ray * 3 + c);
    }
  };
  auto prefetch = [&](int64_t grp) {
    if constexpr (!EMBEDDED) {
      prefetch_round(grp, 0);
      if constexpr (T > 4) {      // the fifth tile: 16 lanes (a staging row holds exactly the wave's 16 T samples)
        if (lane < 16 * (T - 4)) prefetch_round(grp, 4);
      }
    }
  };
  auto staged = [&](int t, int slot) -> float {
    return *reinterpret_cast<const float __attribute__((address_space(3)))*>(
        static_cast<uintptr_t>(stage_base + slot * kStageRow + (t * 16 + n) * 4));
  };

  // group order of a workgroup: sg consecutive groups (one, unless rays span several chunks), then a jump of gridDim.x such runs
  const int sg = a.sg_groups > 1 ? a.sg_groups : 1;
  auto group_after = [&](int64_t grp_, int gi_) -> int64_t {
    return gi_ + 1 == sg ? grp_ + static_cast<int64_t>(gridDim.x - 1) * sg + 1 : grp_ + 1;
  };
  prefetch(static_cast<int64_t>(blockIdx.x) * sg);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uint32_t par = 0;      // parity of the group pass: which {z, dist} record buffer this group writes (compositing only)
  int gi = 0;            // position of the group in its run
  for (int64_t grp = static_cast<int64_t>(blockIdx.x) * sg, nxt_grp = 0; grp < n_groups;
       grp = nxt_grp, gi = (gi + 1 == sg ? 0 : gi + 1), par ^= 1u) {
    nxt_grp = group_after(grp, gi);
    Block xe[T][2];   // embedded point (63 -> 64 features); registers for layer 0 only
    // Non-finite inputs: the reference's arithmetic turns a NaN / inf coordinate into NaN in all four outputs (sin / cos,
    // nn.Linear and torch.relu all propagate it).  Here the packed-int16 ReLU would drop the NEGATIVE NaNs the matrix
    // cores produce, so the samples are flagged (bit t of `bad`, one register across the network) and written as NaN.
    uint32_t bad = 0;
    [[maybe_unused]] bool rec_finite = true;   // render kernel: the {z, dist |d|} records of this lane's samples are finite
    auto finite = [](float v) { return __builtin_fabsf(v) < __builtin_inff(); };
    asm volatile("" ::: "memory");   // the staged inputs landed several slab steps ago (in-order vmcnt)
    if constexpr (EMBEDDED) {
      static_for<T>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        Block ve[1];    // embedded view direction (27 -> 32)
        bool valid;
        const float* row = a.x90 + sample_of(grp, t, n, valid) * a.x_stride;
        gather3_16<M, 10, 2>(xe[t], row, g);
        bool ok = finite(row[0]) && finite(row[1]) && finite(row[2]);
        if (a.use_viewdirs) {
          gather3_16<M, 4, 1>(ve, row + 63, g);
          ok = ok && finite(row[63]) && finite(row[64]) && finite(row[65]);
        }
        if (!ok) bad |= 1u << t;
        stash_put(t, 0, xe[t][0]); stash_put(t, 1, xe[t][1]);
        if (a.use_viewdirs) stash_put(t, 2, ve[0]);
      });
    } else {
      // All staged values of the wave's four tiles come out of LDS in ONE burst (40 reads, one wait) before anything is
      // embedded or stashed: read tile by tile, each read sat right in front of its first use (an exposed LDS latency per
      // value, ~3 % of the kernel: nothing else runs on this SIMD while the lone wave waits).
      float P[T][3], V[T][3];          // (compile-time indices only: a runtime index would park the arrays in scratch)
      if (a.comp) {   // (wave-uniform) placement and the {z, dist} records, one sample per lane (ns_comp_epilogue.h)
        nsepi::place_wave(a, rec, [&](int slot, int i) -> float {
          return *reinterpret_cast<const float __attribute__((address_space(3)))*>(
              static_cast<uintptr_t>(stage_base + slot * kStageRow + i * 4));
        }, grp, gi, par, wave);
      }
      static_for<T>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        if (a.pts) {
          static_for<3>([&](auto c_) { P[t][decltype(c_)::value] = staged(t, decltype(c_)::value); });
        } else {
          float zz;
          if constexpr (kRenderTU) {   // (always composites) the whole record: a non-finite dist could turn a zero alpha into NaN
            const nsepi::v2f zdr = *rec.zd(par, (wave * T + t) * 16 + n);
            zz = zdr.x;
            rec_finite = rec_finite && finite(zdr.x) && finite(zdr.y);
          } else {
            zz = a.comp ? (*rec.zd(par, (wave * T + t) * 16 + n)).x : staged(t, 6);
          }
          static_for<3>([&](auto c_) {
            constexpr int c = decltype(c_)::value;
            P[t][c] = staged(t, c) + staged(t, 3 + c) * zz;
          });
        }
        static_for<3>([&](auto c_) {
          constexpr int c = decltype(c_)::value;
          V[t][c] = a.use_viewdirs ? staged(t, 7 + c) : 0.0f;
        });
      });
      asm volatile("" ::: "memory");   // ... and only then the stash writes below (the compiler cannot tell the two LDS regions apart)
      // A view direction is embedded once per RUN of tiles that share it (a wave's consecutive samples lie on one ray when
      // N is a multiple of 64 and the wave has four tiles, on at most two when it has five): tile t reuses the previous
      // tile's embedding when its direction compares equal BY VALUE, wave-uniformly; a NaN compares unequal and is embedded.
      bool new_view[T];
      static_for<T>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        if constexpr (t == 0) {
          new_view[0] = true;
        } else {
          const bool same = V[t][0] == V[t - 1][0] && V[t][1] == V[t - 1][1] && V[t][2] == V[t - 1][2];
          new_view[t] = __builtin_amdgcn_ballot_w64(same) != ~0ull;
        }
      });
      Block ve0[1];
      static_for<T>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        bool ok = finite(P[t][0]) && finite(P[t][1]) && finite(P[t][2]);
        embed3_16<M, false, 10, 2>(xe[t], P[t][0], P[t][1], P[t][2], g);
        stash_put(t, 0, xe[t][0]); stash_put(t, 1, xe[t][1]);
        if (a.use_viewdirs) {
          ok = ok && finite(V[t][0]) && finite(V[t][1]) && finite(V[t][2]);
          if (new_view[t]) embed3_16<M, false, 4, 1>(ve0, V[t][0], V[t][1], V[t][2], g);   // (wave-uniform branch)
          stash_put(t, 2, ve0[0]);
        }
        if (!ok) bad |= 1u << t;
      });
    }

    const float* bias = bias_lds;
    Block hA[T][NKB], hB[T][NKB];
    f32x4a last[T];
    auto in_x = [&](auto t_, auto kb_) -> const Block& { return xe[decltype(t_)::value][decltype(kb_)::value]; };
    auto in_A = [&](auto t_, auto kb_) -> const Block& { return hA[decltype(t_)::value][decltype(kb_)::value]; };
    auto in_B = [&](auto t_, auto kb_) -> const Block& { return hB[decltype(t_)::value][decltype(kb_)::value]; };
    // The skip layer sees cat[x, h]: the embedded point comes back from the per-wave LDS stash ONCE per layer into
    // registers (32 of them, live for that layer only) instead of once per 16-row sub-block -- 8 reads instead of 128
    // per wave pass, none of them right in front of the MFMA that needs it.
    Block xs[T][2];
    auto load_xs = [&] {
      static_for<T>([&](auto t_) {
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

    // layer 0: x -> hA
    if constexpr (PROD) {
      prefetch(nxt_grp);
      layer0_asm<M, T>(ring, bias, g, xe, hA); bias += NSB * 16;
    } else
    { layer_ob16<M, T, NSB, 2, true>(ring, bias, g, hA, last, in_x); convert_last16<M, true, T, NSB>(hA, last); bias += NSB * 16; }
    // next group's inputs (clamped to the last sample past the end: loaded, never used); this group's staged values
    // have been consumed (they fed the embeddings above)
    if constexpr (!PROD) prefetch(nxt_grp);   // (PROD asked before layer 0: compiled code between two statements costs register copies)
    int l = 1;
    [[maybe_unused]] uint32_t kb_dead = 0, kb_mask7 = 0;   // K-block-skipping kernel: steps jumped over; the trunk output's live mask
    if constexpr (PROD) {
      static_assert(NKB == 8 && (T == 4 || T == 5) && NWAVES == 4, "the generated streams are W = 256, four or five tiles, four waves");
      hidden_layer_asm<M, T, true, false>(ring, bias, g, hA, hB, xs); bias += NSB * 16;    // 1
      hidden_layer_asm<M, T, false, false>(ring, bias, g, hA, hB, xs); bias += NSB * 16;   // 2
#ifdef NS_OB16_TU_KMASK
      // live masks of the tested K-blocks travel from each layer to the next in an SGPR; `dead` counts the steps jumped over
      static_assert(T == 5, "the K-block-skipping statements are five-tile");
      constexpr uint32_t kAll = (1u << kKbsMaskBits) - 1u;
#ifdef NS_OB16_TU_KSUFFIX
      auto dead_of = [&](uint32_t m) { return static_cast<uint32_t>(__builtin_ctz(m | (1u << kKbsMaskBits))); };   // the body's d
#else
      auto dead_of = [&](uint32_t m) { return static_cast<uint32_t>(__builtin_popcount(~m & kAll)); };
#endif
      uint32_t km = kbs_hidden_layer_asm<M, 0, true>(ring, bias, g, hA, hB, xs, kAll); bias += NSB * 16;    // 3
      kb_dead += NSB * dead_of(km);
      km = kbs_hidden_layer_asm<M, 1, false>(ring, bias, g, hA, hB, xs, km); bias += NSB * 16;             // 4
      kb_dead += NSB * dead_of(km);
      load_xs();
      km = kbs_hidden_layer_asm<M, 2, true>(ring, bias, g, hA, hB, xs, km); bias += NSB * 16;              // 5: cat[x, h]
      kb_dead += NSB * dead_of(km);
      km = kbs_hidden_layer_asm<M, 1, false>(ring, bias, g, hA, hB, xs, km); bias += NSB * 16;             // 6
      kb_dead += NSB * dead_of(km);
      km = kbs_hidden_layer_asm<M, 3, true>(ring, bias, g, hA, hB, xs, km); bias += NSB * 16;              // 7: the trunk's output is in hB
      kb_mask7 = km;
#else
      hidden_layer_asm<M, T, true, false>(ring, bias, g, hA, hB, xs); bias += NSB * 16;    // 3
      hidden_layer_asm<M, T, false, false>(ring, bias, g, hA, hB, xs); bias += NSB * 16;   // 4
      load_xs();
      hidden_layer_asm<M, T, true, true>(ring, bias, g, hA, hB, xs); bias += NSB * 16;     // 5: cat[x, h]
      hidden_layer_asm<M, T, false, false>(ring, bias, g, hA, hB, xs); bias += NSB * 16;   // 6
      hidden_layer_asm<M, T, true, false>(ring, bias, g, hA, hB, xs); bias += NSB * 16;    // 7: the trunk's output is in hB
#endif
      l = 8;
    }
    // layers 1 .. D-1, two per trip (hA -> hB -> hA); the layer after `skip` sees cat[x, h]
    if constexpr (!PROD) {
    for (; l + 1 < a.D; l += 2) {
      if ((a.skip_mask >> (l - 1)) & 1u) { load_xs(); layer_ob16<M, T, NSB, NKB + 2, true>(ring, bias, g, hB, last, in_xA); }
      else layer_ob16<M, T, NSB, NKB, true>(ring, bias, g, hB, last, in_A);
      convert_last16<M, true, T, NSB>(hB, last); bias += NSB * 16;
      if ((a.skip_mask >> l) & 1u) { load_xs(); layer_ob16<M, T, NSB, NKB + 2, true>(ring, bias, g, hA, last, in_xB); }
      else layer_ob16<M, T, NSB, NKB, true>(ring, bias, g, hA, last, in_B);
      convert_last16<M, true, T, NSB>(hA, last); bias += NSB * 16;
    }
    if (l < a.D) {  // odd layer left over: hA -> hB, then move back
      if ((a.skip_mask >> (l - 1)) & 1u) { load_xs(); layer_ob16<M, T, NSB, NKB + 2, true>(ring, bias, g, hB, last, in_xA); }
      else layer_ob16<M, T, NSB, NKB, true>(ring, bias, g, hB, last, in_A);
      convert_last16<M, true, T, NSB>(hB, last); bias += NSB * 16;
      static_for<T>([&](auto t_) { static_for<NKB>([&](auto b_) { hA[decltype(t_)::value][decltype(b_)::value] = hB[decltype(t_)::value][decltype(b_)::value]; }); });
    }
    }
    if (!PROD && !a.use_viewdirs) {
      // output_linear (W -> out_ch, no activation, run_nerf_helpers.py:132-133): ONE 16-row sub-block whose raw accumulators
      // come back in `last`: row 4 g + r sits in register r of lane group g
      layer_ob16<M, T, 1, NKB, kNone>(ring, bias, g, hB, last, in_A);
      static_for<T>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        bool valid;
        const int64_t sidx = sample_of(grp, t, n, valid);
        static_for<4>([&](auto r_) {
          constexpr int r = decltype(r_)::value;
          const int row = 4 * g + r;
          if (valid && row < a.out_ch) a.raw[sidx * a.out_ch + row] = ((bad >> t) & 1u) ? __builtin_nanf("") : last[t][r];
        });
      });
      continue;
    }
    // views o feature (folded at pack time: feature_linear has no activation, run_nerf_helpers.py:119-125) on
    // cat[h, dirs27] -> W/2, relu: (hA, ve) -> hB[0 .. NKB/2); alpha_linear rides along as row 0 of one extra, LAST
    // sub-block, whose raw accumulators come back in `last`: sigma = row 0 (lane group 0, register 0)
    Block vs[T];   // the embedded view direction, once for the layer's 9 sub-blocks
    static_for<T>([&](auto t_) { vs[decltype(t_)::value] = stash_get(decltype(t_)::value, 2); });
    auto in_Av = [&](auto t_, auto kb_) -> const Block& {
      constexpr int kb = decltype(kb_)::value;
      if constexpr (kb < NKB) return hA[decltype(t_)::value][kb]; else return vs[decltype(t_)::value];
    };
    float sigma[T];
    [[maybe_unused]] bool skipped = false;   // render kernel: this wave ran the drain twins
    if constexpr (PROD) {   // the trunk ended in hB: (hB, ve) -> hA[0 .. NKB/2), then rgb from hA
      auto in_Bv = [&](auto t_, auto kb_) -> const Block& {
        constexpr int kb = decltype(kb_)::value;
        if constexpr (kb < NKB) return hB[decltype(t_)::value][kb]; else return vs[decltype(t_)::value];
      };
      (void)in_Bv;
#ifdef NS_OB16_TU_RENDER
      // the sigma-first stream: sigma, then EITHER colour and rgb OR their drain twins (see the file's header comment)
      u32x4 D[T];
      static_for<T>([&](auto t_) { D[decltype(t_)::value] = __builtin_bit_cast(u32x4, vs[decltype(t_)::value].v); });
#ifdef NS_OB16_TU_KMASK
#ifdef NS_OB16_TU_KSUFFIX
      const uint32_t dead7 = static_cast<uint32_t>(__builtin_ctz(kb_mask7 | (1u << kKbsMaskBits)));
#else
      const uint32_t dead7 = static_cast<uint32_t>(__builtin_popcount(~kb_mask7 & ((1u << kKbsMaskBits) - 1u)));
#endif
      kbs_sigma_asm<M>(ring, bias, g, hB, D, sigma, kb_mask7); bias += 16;
      kb_dead += dead7;
#else
      render_sigma_asm<M, T>(ring, bias, g, hB, D, sigma); bias += 16;
#endif
      // (bitwise, not ||: straight-line code) this lane knows of a sample that may contribute, or that must come out NaN
      uint32_t live = static_cast<uint32_t>(bad != 0) | static_cast<uint32_t>(!rec_finite);
      static_for<T>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        // lanes 0..15 hold row 0 = sigma; a NaN compares false, -0 <= 0
        live |= static_cast<uint32_t>(g == 0) & static_cast<uint32_t>(!(sigma[t] <= 0.0f));
      });
      skipped = __builtin_amdgcn_ballot_w64(live != 0) == 0;   // (wave-uniform: a scalar branch)
      if (skipped) {
        render_drain_asm_run<M, T, 3>(ring, bias, g); bias += (NSB / 2) * 16;
        render_drain_asm_run<M, T, 4>(ring, bias, g);
        static_for<T>([&](auto t_) { last[decltype(t_)::value] = f32x4a{0.0f, 0.0f, 0.0f, 0.0f}; });
      } else {
#ifdef NS_OB16_TU_KMASK
        kbs_colour_asm<M>(ring, bias, g, hB, D, hA, kb_mask7); bias += (NSB / 2) * 16;
        kb_dead += (NSB / 2) * dead7;
#else
        render_colour_asm<M, T>(ring, bias, g, hB, D, hA); bias += (NSB / 2) * 16;
#endif
        render_rgb_asm<M, T>(ring, bias, g, hA, last);
      }
#else
      views_asm<M, T>(ring, bias, g, hB, vs, hA, last); bias += (NSB / 2 + 1) * 16;
      static_for<T>([&](auto t_) { sigma[decltype(t_)::value] = last[decltype(t_)::value][0]; });
      rgb_asm<M, T>(ring, bias, g, hA, last);
#endif
    } else {
    layer_ob16<M, T, NSB / 2 + 1, NKB + 1, kRelu>(ring, bias, g, hB, last, in_Av); bias += (NSB / 2 + 1) * 16;
    static_for<T>([&](auto t_) { sigma[decltype(t_)::value] = last[decltype(t_)::value][0]; });
    // rgb (W/2 -> 3): rows 0..2 (lane group 0, registers 0..2)
    layer_ob16<M, T, 1, NKB / 2, kNone>(ring, bias, g, hA, last, in_B);
    }

    bool comp = false;
    if constexpr (!EMBEDDED) comp = a.comp != 0;
    const int le = nsepi::opaque_lane();      // the lane id of the epilogue (see nsepi::opaque_lane)
    if (le < 16) {                     // lane group g == 0 holds the outputs: rows 0..2 = rgb, sigma from the view layer
      static_for<T>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        bool valid;
        const int64_t sidx = sample_of(grp, t, le, valid);
        float4 o4 = make_float4(last[t][0], last[t][1], last[t][2], sigma[t]);
        if ((bad >> t) & 1u) { const float q = __builtin_nanf(""); o4 = make_float4(q, q, q, q); }
        if (comp) *rec.raw((wave * T + t) * 16 + le) = v4f{o4.x, o4.y, o4.z, o4.w};
        if (valid && a.raw) reinterpret_cast<float4*>(a.raw)[sidx] = o4;
      });
    }
    if constexpr (kRenderTU) {
      if (skipped && a.skip_count && le == 0) atomicAdd(a.skip_count, 1u);
#ifdef NS_OB16_TU_KSUFFIX
      if (kb_dead && a.skip_count && le == 0) atomicAdd(a.skip_count + 2, kb_dead);
#elif defined(NS_OB16_TU_KBSKIP)
      if (kb_dead && a.skip_count && le == 0) atomicAdd(a.skip_count + 1, kb_dead);
#endif
    }
    if constexpr (!EMBEDDED) nsepi::composite_group(a, rec, comp, grp, gi, par, wave, le);
  }
  ring.finish();
}

template <class M, int NKB, bool EMB, bool PROD = false, int TT = kT>
int launch(Nerf16Args& a, hipStream_t stream) {
  const int64_t n_tiles = (a.S + 15) / 16;
  const int64_t n_groups = (n_tiles + kWaves * TT - 1) / (kWaves * TT);
  a.sg_groups = nsepi::run_groups(kWaves * TT * 16, a.m_chunks, a.N);
  const int64_t n_runs = (n_groups + a.sg_groups - 1) / a.sg_groups;
  const Ob16Lds<TT> lm(a.bias_floats, a.comp && !EMB ? nsepi::Records<TT, kWaves>::kBytes : 0);
  return ns::launch_persistent("ns_nerf_forward", NS_OB16_KERNEL<M, NKB, EMB, PROD, TT>, a, kWaves * 64, lm.end, n_runs, stream);
}

#ifdef NS_OB16_TU_MAIN
// Which launches the render kernel takes (five tiles): the handle carries the sigma-first stream (a production 16-bit network),
// the kernel composites rays of one chunk, and nothing handed out reads raw rgb of a sample whose weight may be zero -- raw
// itself, the max-weight sample, the every-ray and the selective guard.  Per-sample weights / z / pts do not disqualify.
bool render_eligible(const ns_weights* net, const Nerf16Args& a) {
  return net->stream2_dev && net->bias2_dev && !ns::debug_flags().no_colour_skip && a.comp != 0 && !a.m_chunks && a.N >= 2 &&
         a.N <= 64 && (a.N & (a.N - 1)) == 0 && !a.raw && !a.pts && !a.x90 && !a.max_w && !a.max_z && !a.max_rgb && !a.fix_rec &&
         !a.sig_last;
}
template <class M, bool EMB>
int dispatch_m(const ns_weights* net, Nerf16Args& a, hipStream_t stream) {
#if NS_NERF16_T == 4 && NS_NERF16_WAVES == 4
  if (net->width == 256 && net->depth == 8 && net->skip_mask == (1u << 4) && net->use_viewdirs && !ns::debug_flags().generic_kernels) {
    // the production network: hand-scheduled layers, four or five 16-sample tiles per wave.  Five tiles read 20 % fewer
    // weight fragments and refill bytes per sample (-2.5 % per frame on the final build, profiles/r03c_ab_tiles_final_build.log);
    // the persistent grid runs ceil(groups / CUs) rounds of 256 (320) samples per workgroup, so the choice is made per
    // launch on the rounds' total: a 32768-ray x 64 chunk is exactly 32 rounds of four tiles but 25.6 -> 26 of five.
    int cus = ns::cu_count();
    if (cus <= 0) cus = 256;
    auto rounds = [&](int64_t per_group) { const int64_t g = (a.S + per_group - 1) / per_group; return (g + cus - 1) / cus; };
    const double t4 = static_cast<double>(rounds(kWaves * 4 * 16)) * 4.0, t5 = static_cast<double>(rounds(kWaves * 5 * 16)) * 5.0 * 0.975;
    int tiles = NS_OB16_PROD_T ? NS_OB16_PROD_T : (t5 < t4 ? 5 : 4);
    if (ns::prod_tiles_hint()) tiles = ns::prod_tiles_hint();               // the renderer's hint (host copies in flight)
    if (ns::debug_flags().prod_tiles) tiles = ns::debug_flags().prod_tiles;   // diagnostic override (ns_debug_set)
    if (tiles == 5) {
      if (!EMB && render_eligible(net, a)) {
        Nerf16Args r = a;
        r.stream = static_cast<const char*>(net->stream2_dev); r.bias = net->bias2_dev;
        // the K-block-skipping twin (opt-in): same launches, same stream; a handle with a non-finite weight stays on the render kernel
        if (net->kbskip_ok && ns::debug_flags().kblock_skip) return nsob16::launch_kbskip_t5(M::kDtype, r, stream);
        // the dead-suffix twin: 1 every such handle, 2 only those packed with the unit order (where dead blocks are a suffix)
        const int ksuffix = ns::debug_flags().kblock_suffix;
        if (net->kbskip_ok && (ksuffix == 1 || (ksuffix == 2 && net->unit_ordered))) return nsob16::launch_ksuffix_t5(M::kDtype, r, stream);
        return nsob16::launch_render_t5(M::kDtype, r, stream);
      }
      return nsob16::launch_prod_t5(M::kDtype, EMB, a, stream);
    }
    return launch<M, 8, EMB, true, 4>(a, stream);
  }
#endif
  return net->width == 256 ? launch<M, 8, EMB>(a, stream) : launch<M, 4, EMB>(a, stream);
}
#endif

}  // namespace

#if defined(NS_OB16_TU_KSUFFIX)
int nsob16::launch_ksuffix_t5(int dtype, Nerf16Args& a, hipStream_t stream) {
  if (dtype == Mma16BF16::kDtype) return launch<Mma16BF16, 8, false, true, 5>(a, stream);
  return launch<Mma16F16, 8, false, true, 5>(a, stream);
}
#elif defined(NS_OB16_TU_KBSKIP)
int nsob16::launch_kbskip_t5(int dtype, Nerf16Args& a, hipStream_t stream) {
  if (dtype == Mma16BF16::kDtype) return launch<Mma16BF16, 8, false, true, 5>(a, stream);
  return launch<Mma16F16, 8, false, true, 5>(a, stream);
}
#elif defined(NS_OB16_TU_RENDER)
int nsob16::launch_render_t5(int dtype, Nerf16Args& a, hipStream_t stream) {
  if (dtype == Mma16BF16::kDtype) return launch<Mma16BF16, 8, false, true, 5>(a, stream);
  return launch<Mma16F16, 8, false, true, 5>(a, stream);
}
#elif defined(NS_OB16_TU_T5)
int nsob16::launch_prod_t5(int dtype, bool embedded, Nerf16Args& a, hipStream_t stream) {
  if (dtype == Mma16BF16::kDtype) return embedded ? launch<Mma16BF16, 8, true, true, 5>(a, stream) : launch<Mma16BF16, 8, false, true, 5>(a, stream);
  return embedded ? launch<Mma16F16, 8, true, true, 5>(a, stream) : launch<Mma16F16, 8, false, true, 5>(a, stream);
}
#else
// which (network, sample count) pairs the kernel composites itself (see nsepi::CompFields::comp): the 16-bit fields here, the split-fp16
// (f16x3) fields in ns_nerf_mlp_x3.hip
bool ns_nerf_can_composite(const ns_weights* net, int N) {
  return net && net->kind == NS_KIND_NERF && net->layout == 16 &&
         (net->dtype == NS_DTYPE_BF16 || net->dtype == NS_DTYPE_F16 || net->dtype == NS_DTYPE_F16X3) &&
         net->use_viewdirs && net->out_ch == 4 &&
         ((N >= 2 && N <= 64 && (N & (N - 1)) == 0) || (N > 64 && N % 64 == 0 && N <= 512));
}

// called by ns_nerf_forward / ns_nerf_forward_embedded for handles packed with layout 16 (arguments validated there)
int ns_nerf_forward_ob16(const ns_weights* net, const float* pts_dev, const float* o_dev, const float* d_dev,
                         const float* z_dev, const float* viewdirs_dev, const float* x90_dev, int64_t S, int N,
                         float* raw_dev, hipStream_t stream, const ns_composite_args* comp) {
  if (comp) {
    if (!ns_nerf_can_composite(net, N)) {
      ns::set_error("in-kernel compositing needs a bf16, f16 or f16x3 NeRF handle with view directions and N a power of two in "
                    "[2, 64] or a multiple of 64 up to 512 (N = %d)", N);
      return NS_E_UNSUPPORTED;
    }
    if (pts_dev || x90_dev || !(o_dev && d_dev) || !(z_dev || comp->mean_dev) || !(comp->rgb_dev && comp->disp_dev)) {
      ns::set_error("in-kernel compositing needs rays (o, d), depths (z or mean) and the rgb / disp outputs");
      return NS_E_INVALID;
    }
  }
  if (net->dtype == NS_DTYPE_F16X3)   // split fp16 operands: ns_nerf_mlp_x3.hip
    return ns_nerf_forward_x3(net, pts_dev, o_dev, d_dev, z_dev, viewdirs_dev, x90_dev, S, N, raw_dev, stream, nullptr, comp);
  const int slabs = ob16_field_slabs(1, net->width, net->depth, net->skip_mask, net->use_viewdirs);
  if (slabs != static_cast<int>(net->n_slabs)) {
    ns::set_error("ns_nerf_forward: packed stream has %u slabs, kernel program expects %d", net->n_slabs, slabs);
    return NS_E_INVALID;
  }
  Nerf16Args a{};
  set_field_args(a, net, pts_dev, o_dev, d_dev, z_dev, viewdirs_dev, x90_dev, S, N, raw_dev);
  if (comp) {
    nsepi::set_comp_args(a, comp, N);
    if (comp->fix_rec_dev) {
      if (comp->sigma_last_dev || comp->max_w_dev) {
        ns::set_error("the selective guard excludes the every-ray guard's sigma array and the max-weight sample");
        return NS_E_INVALID;
      }
      a.fix_thr = comp->fix_thr; a.fix_count = comp->fix_count_dev; a.fix_rec = comp->fix_rec_dev;
    }
  }
  // the render kernel's skip counter: NULL unless ns_debug_set("count_colour_skips", 1); zeroed for EVERY launch from here, so a
  // launch that runs another kernel reads back as 0
  const int rc_count = ns::colour_skip_counter(&a.skip_count, stream);
  if (rc_count != NS_OK) return rc_count;
  const bool emb = x90_dev != nullptr;
#ifdef NS_OB16_VARIANT_BUILD   // tools/build_asm_variant.sh: only the kernel under test is instantiated (a 20 s build)
  if (net->dtype == NS_DTYPE_BF16 && !emb && net->width == 256 && net->depth == 8 && net->skip_mask == (1u << 4) && net->use_viewdirs)
    return launch<Mma16BF16, 8, false, true, (NS_OB16_PROD_T ? NS_OB16_PROD_T : 4)>(a, stream);
  return NS_E_UNSUPPORTED;
#endif
  if (net->dtype == NS_DTYPE_BF16) return emb ? dispatch_m<Mma16BF16, true>(net, a, stream) : dispatch_m<Mma16BF16, false>(net, a, stream);
  if (net->dtype == NS_DTYPE_F16) return emb ? dispatch_m<Mma16F16, true>(net, a, stream) : dispatch_m<Mma16F16, false>(net, a, stream);
  return NS_E_UNSUPPORTED;
}
#endif  // NS_OB16_TU_RENDER / NS_OB16_TU_T5 / main
