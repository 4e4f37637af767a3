// Tall GEMM of the field fit (autograd.NerfFunction with engine="tall"): the layer forwards y = act(x W^T + b) and the
// grad-input products dx = (dy W) * act'(y) over `rows` samples, where rows is the batch of a NeRF step (1024 rays x 64 .. 192
// samples = 65 536 .. 196 608) and N, K <= 512:
//   C[i, j] (+)= sum_k A[i, k] B[j, k] (+ bias[j]),  then act, then dact          (the epilogues of ns_gemm_fused)
//
// ns_gemm_fused gives one workgroup one 32 x 32 output tile: at N = 256 every row of A is fetched eight times.  Here a
// workgroup owns a SLAB of 128 rows and ALL N columns of it, so a row of A is fetched once per call; B (<= 1 MiB) is the
// operand that is re-read, once per slab, through L2 and LDS.  grid = one workgroup per slab.
//   * four row groups of 32 rows x CG column groups (CG = 2 above 256 columns: 512 threads); a wave holds NT accumulator
//     tiles of 32 x 32 (v_mfma_f32_32x32x2_f32: exact fp32 products), NT = ceil(ceil(N / 32) / CG) <= 8: at most 128
//     accumulator registers;
//   * K is walked in chunks of 16.  A chunk of A [128 x 16] and of B [N x 16] goes global -> registers -> LDS, k-major
//     (As[k][row], Bs[k][col], row pitch = 2 mod 32: no bank conflict on the way in): the loads of chunk c + 1 are issued
//     before the MFMAs of chunk c and fly under them; the LDS holds one chunk (two barriers per chunk, <= 25 KiB), so two
//     workgroups share a CU at N = 256 and cover each other's barriers.  Loads are single dwords, a 64-B row segment per
//     16 lanes: the fit passes column slices of the cat[xe, h] buffer, which are 4-byte aligned only;
//   * step e of a chunk feeds lane (r, h) the k value e + 8 h: a half-wave reads 32 consecutive floats of one k-row of LDS
//     (no bank conflict on the way out).  k past K is a zero in both operands.
// The order of the sum over k is a function of K alone -- not of rows, the grid or the device: the same bits on every call
// and every stream.  No atomics.
#include "ns_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SLAB = 128;             // rows per workgroup: 4 row groups of 32
constexpr int KC = 16;                // k values per chunk
constexpr int KH = KC / 2;            // MFMA steps per chunk
constexpr int A_PITCH = SLAB + 2;     // = 2 mod 32: the half-wave that stores 16 k values of 2 rows hits 32 banks

struct TallArgs {
  const float* A; int64_t lda;
  const float* B; int64_t sb0, sb1;
  const float* bias;
  float* C; int64_t ldc;
  int64_t rows;
  int N, K;
  int accumulate, act, dact;
  const float* dref; int64_t ld_ref;
};

template <int NT, int CG, bool JFAST>
__global__ void __launch_bounds__(256 * CG, 2 / CG)
gemm_tall_kernel(const TallArgs p) {
  constexpr int NTHREADS = 256 * CG;
  constexpr int NCOLS = 32 * NT * CG;               // columns the workgroup holds (>= N)
  constexpr int B_PITCH = NCOLS + 2;
  constexpr int A_LOADS = SLAB * KC / NTHREADS;     // dwords per thread and chunk
  constexpr int B_LOADS = NCOLS * KC / NTHREADS;
  __shared__ float As[KC * A_PITCH];
  __shared__ float Bs[KC * B_PITCH];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int rg = wave & 3, cg = wave >> 2;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * SLAB;
  const int nvalid = static_cast<int>(p.rows - row0 < SLAB ? p.rows - row0 : SLAB);    // rows of this slab, >= 1
  constexpr bool jfast = JFAST;                     // B contiguous along j (the W^T view of grad-input): lanes walk j

  // Element `flat` = i * NTHREADS + tid of a chunk: A -> (row = flat / 16, k = flat % 16); B -> (j = flat / 16, k = flat % 16),
  // or with jfast (k = flat / NCOLS, j = flat % NCOLS).  A load's address is a workgroup-uniform base, advanced by the chunk,
  // plus a 32-bit byte offset that does not change from chunk to chunk.  A row past the slab's last and a column past N are
  // read from the last valid one: they feed output rows / columns that are never stored.  k past K is a zero in both
  // operands: only the last chunk can hold one, and it predicates its loads.
  uint32_t offa[A_LOADS], offb[B_LOADS];
#pragma unroll
  for (int i = 0; i < A_LOADS; ++i) {
    const int flat = i * NTHREADS + tid;
    offa[i] = 4u * (static_cast<uint32_t>(min(flat >> 4, nvalid - 1)) * static_cast<uint32_t>(p.lda) + (flat & 15));
  }
#pragma unroll
  for (int i = 0; i < B_LOADS; ++i) {
    const int flat = i * NTHREADS + tid;
    const int j = min(jfast ? flat % NCOLS : flat >> 4, p.N - 1);
    const int kk = jfast ? flat / NCOLS : flat & 15;
    offb[i] = 4u * (static_cast<uint32_t>(j) * static_cast<uint32_t>(p.sb0) + static_cast<uint32_t>(kk) * static_cast<uint32_t>(p.sb1));
  }
  const char* abase = reinterpret_cast<const char*>(p.A + row0 * p.lda);
  const char* bbase = reinterpret_cast<const char*>(p.B);

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;

  float ra[A_LOADS], rb[B_LOADS];
  auto load = [&](int k0) {
    const char* a0 = abase + 4 * static_cast<int64_t>(k0);
    const char* b0 = bbase + 4 * static_cast<int64_t>(k0) * p.sb1;
    if (k0 + KC <= p.K) {                           // (workgroup-uniform)
#pragma unroll
      for (int i = 0; i < A_LOADS; ++i) ra[i] = *reinterpret_cast<const float*>(a0 + offa[i]);
#pragma unroll
      for (int i = 0; i < B_LOADS; ++i) rb[i] = *reinterpret_cast<const float*>(b0 + offb[i]);
    } else {
      const int left = p.K - k0;                    // 1 .. KC - 1 values of k in the last chunk
#pragma unroll
      for (int i = 0; i < A_LOADS; ++i) ra[i] = (tid & 15) < left ? *reinterpret_cast<const float*>(a0 + offa[i]) : 0.f;
#pragma unroll
      for (int i = 0; i < B_LOADS; ++i) {
        const int flat = i * NTHREADS + tid;
        const int kk = jfast ? flat / NCOLS : flat & 15;
        rb[i] = kk < left ? *reinterpret_cast<const float*>(b0 + offb[i]) : 0.f;
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {
      const int flat = i * NTHREADS + tid;
      As[(flat & 15) * A_PITCH + (flat >> 4)] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
      const int flat = i * NTHREADS + tid;
      const int j = jfast ? flat % NCOLS : flat >> 4;
      const int kk = jfast ? flat / NCOLS : flat & 15;
      Bs[kk * B_PITCH + j] = rb[i];
    }
  };

  const float* ap = As + KH * h * A_PITCH + 32 * rg + r;
  const float* bp = Bs + KH * h * B_PITCH + 32 * NT * cg + r;
  load(0);
  for (int k0 = 0; k0 < p.K; k0 += KC) {
    __syncthreads();                                // the MFMAs of the chunk before have read the LDS
    stage();
    __syncthreads();
    if (k0 + KC < p.K) load(k0 + KC);               // in flight under this chunk's MFMAs
#pragma unroll
    for (int e = 0; e < KH; ++e) {
      const float a = ap[e * A_PITCH];
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[e * B_PITCH + 32 * t], acc[t], 0, 0, 0);
    }
  }

  // accumulator register q of lane (r, h): row (q & 3) + 8 (q >> 2) + 4 h of the wave's 32, column r of tile t
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int j = 32 * (NT * cg + t) + r;
    if (j >= p.N) continue;
    const float bj = p.bias ? p.bias[j] : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int lr = 32 * rg + (q & 3) + 8 * (q >> 2) + 4 * h;
      if (lr >= nvalid) continue;
      const int64_t row = row0 + lr;
      float v = acc[t][q];
      if (p.bias) v += bj;
      float* c = p.C + row * p.ldc + j;
      if (p.accumulate) v += *c;
      if (p.act == 1) v = v < 0.f ? 0.f : v;          // NaN stays NaN, as torch.relu (fmaxf would drop it)
      else if (p.act == 2) v = v > 0.f ? v : 0.01f * v;
      else if (p.act == 3) v = 1.f / (1.f + expf(-v));
      if (p.dact) {
        const float y = p.dref[row * p.ld_ref + j];
        v *= p.dact == 1 ? (y > 0.f ? 1.f : 0.f) : p.dact == 2 ? (y > 0.f ? 1.f : 0.01f) : y * (1.f - y);
      }
      *c = v;
    }
  }
}

template <int NT, int CG>
void launch(const TallArgs& a, int64_t slabs, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(slabs));
  if (a.sb1 != 1 && a.sb0 == 1) gemm_tall_kernel<NT, CG, true><<<grid, 256 * CG, 0, st>>>(a);
  else gemm_tall_kernel<NT, CG, false><<<grid, 256 * CG, 0, st>>>(a);
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

extern "C" {

int ns_gemm_tall(const float* A_dev, int64_t lda, const float* B_dev, int64_t sb0, int64_t sb1, const float* bias_dev,
                 float* C_dev, int64_t ldc, int64_t rows, int N, int K, int accumulate, int act, int dact,
                 const float* dact_ref_dev, int64_t ld_ref, void* stream) {
  NS_REQUIRE(rows >= 1 && rows < (static_cast<int64_t>(1) << 31), "rows must be in [1, 2^31)");
  NS_REQUIRE(N >= 1 && K >= 1, "bad shape");
  if (N > 512 || K > 512) {
    ns::set_error("%s: N and K are limited to 512 (got %d x %d)", __func__, N, K);
    return NS_E_UNSUPPORTED;
  }
  NS_REQUIRE(A_dev && B_dev && C_dev, "null pointer");
  NS_REQUIRE(aligned4(A_dev) && aligned4(B_dev) && aligned4(C_dev) && aligned4(bias_dev) && aligned4(dact_ref_dev),
             "pointers must be 4-byte aligned");
  NS_REQUIRE(lda >= K && ldc >= N, "a row stride is shorter than the row");
  // a thread's offset inside a slab of A, and inside B, is kept in 32 bits
  NS_REQUIRE(lda < (1 << 22), "row stride of A too large");
  NS_REQUIRE(sb0 >= 0 && sb1 >= 0 && sb0 < (1 << 19) && sb1 < (1 << 19), "bad stride of B");
  NS_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate is 0 or 1");
  NS_REQUIRE(act >= 0 && act <= 3 && dact >= 0 && dact <= 3, "bad epilogue");
  NS_REQUIRE(dact == 0 || (dact_ref_dev && ld_ref >= N), "dact needs its reference, with a row stride of at least N");
  TallArgs a{};
  a.A = A_dev, a.lda = lda;
  a.B = B_dev, a.sb0 = sb0, a.sb1 = sb1;
  a.bias = bias_dev;
  a.C = C_dev, a.ldc = ldc;
  a.rows = rows, a.N = N, a.K = K;
  a.accumulate = accumulate, a.act = act, a.dact = dact;
  a.dref = dact_ref_dev, a.ld_ref = ld_ref;
  const int64_t slabs = ns::cdiv(rows, SLAB);
  hipStream_t st = ns::as_stream(stream);
  const int tiles = (N + 31) / 32;                  // 1 .. 16
  if (tiles <= 8) {
    switch (tiles) {
      case 1: launch<1, 1>(a, slabs, st); break;
      case 2: launch<2, 1>(a, slabs, st); break;
      case 3: launch<3, 1>(a, slabs, st); break;
      case 4: launch<4, 1>(a, slabs, st); break;
      case 5: launch<5, 1>(a, slabs, st); break;
      case 6: launch<6, 1>(a, slabs, st); break;
      case 7: launch<7, 1>(a, slabs, st); break;
      default: launch<8, 1>(a, slabs, st); break;
    }
  } else {
    switch ((tiles + 1) / 2) {
      case 5: launch<5, 2>(a, slabs, st); break;
      case 6: launch<6, 2>(a, slabs, st); break;
      case 7: launch<7, 2>(a, slabs, st); break;
      default: launch<8, 2>(a, slabs, st); break;
    }
  }
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // extern "C"
