// Grad-weight GEMM of the field fit (autograd.NerfFunction): dW = dy^T x and db = column sums of dy over `rows` samples, where
// rows is the batch of a NeRF step (1024 rays x 64 .. 192 samples = 65 536 .. 196 608) and the output is at most 512 x 512.
//
// ns_gemm_fused gives one workgroup one 32 x 32 output tile and splits the reduction over its four waves only: at these shapes
// that is 64 - 80 workgroups, each wave walking tens of thousands of rows in a serial chain of global-load round trips.  Here
// the ROWS are split over workgroups as well (split-K): grid = output tiles x splits, a pure function of (rows, N, K), sized
// for two workgroups on each of 256 CUs.  A workgroup reduces its slice of rows for one 64 x 64 (N <= 32: 32 x 64) output tile:
//   * both operands are row-major in the reduced index, so a lane (r, h) of the 32x32x2 MFMA reads dy[m + h][n0 + r] and
//     x[m + h][k0 + r]: every operand load of a half-wave is one 128-B row segment, no LDS staging, no barrier in the loop;
//   * a wave holds 2 x 2 (1 x 2) accumulator tiles, so a trip of 16 rows is 32 (24) independent loads for 32 (16) MFMAs; the
//     next trip's loads are issued before this trip's MFMAs, and the four waves of a workgroup (two workgroups per CU) take
//     the trips of the slice in turn: eight chains of trips per CU, each with a whole trip in flight behind ~2048 MFMA cycles;
//   * the four waves' partial tiles are summed through LDS in a fixed order.
// With one split the workgroup writes dW / db itself.  Otherwise it writes its partial tile into a slab of the caller's
// workspace and a second small launch sums the slabs in split order (+ dW when accumulating): no floating-point atomics, the
// same bits on every call.  The db sums ride along in the workgroups of the first output column (k0 = 0), which read dy anyway.
// v_mfma_f32_32x32x2_f32: exact fp32 products, as the rest of the training path.
#include "ns_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WG_ROWS_MIN = 1024;     // rows <= this are never split (the DepthNet-step shapes)
constexpr int WG_TARGET = 512;        // workgroups the split count aims at: two on each of 256 CUs, whatever the device
constexpr int TRIP = 16;              // rows per trip of a wave (8 MFMA steps of 2)

inline int tile_n(int N) { return N <= 32 ? 32 : 64; }

struct WgradShape {
  int tiles_n, tiles_k, splits;
  int64_t chunk;                      // rows per split, a multiple of TRIP
};

inline WgradShape wgrad_shape(int64_t rows, int N, int K) {
  WgradShape s;
  s.tiles_n = (N + tile_n(N) - 1) / tile_n(N);
  s.tiles_k = (K + 63) / 64;
  const int tiles = s.tiles_n * s.tiles_k;
  const int want = (WG_TARGET + tiles - 1) / tiles;
  // at most the power of two at or above rows / 1024: a slice keeps more than 512 rows, and the count changes at 1024 * 2^i + 1
  // rows only
  const int64_t q = ns::cdiv(rows, WG_ROWS_MIN);
  int64_t cap = 1;
  while (cap < q) cap <<= 1;
  s.splits = static_cast<int>(cap < want ? cap : want);
  if (s.splits < 1) s.splits = 1;
  s.chunk = ns::cdiv(ns::cdiv(rows, s.splits), TRIP) * TRIP;
  return s;
}

struct WgradArgs {
  const float* dy; int64_t sdy0, sdy1;
  const float* x; int64_t sx0;
  int64_t rows, chunk;
  int N, K, tiles_k;
  float* out; int64_t ldo, slab;      // split s writes out + s * slab, leading dimension ldo
  float* db; int64_t db_slab;         // db + s * db_slab, or null
  int accumulate;
};

template <int TA>
__global__ void __launch_bounds__(256, 2)
wgrad_kernel(const WgradArgs p) {
  __shared__ float red[4][16][64];
  __shared__ float asum_s[4][TA][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int tk = blockIdx.x % p.tiles_k, tn = blockIdx.x / p.tiles_k;
  const int n0 = tn * 32 * TA, k0 = tk * 64;
  const int split = blockIdx.y;
  const bool want_db = p.db != nullptr && tk == 0;
  int64_t beg = split * p.chunk;
  if (beg > p.rows) beg = p.rows;
  const int64_t end = beg + p.chunk < p.rows ? beg + p.chunk : p.rows;
  const int64_t ntrips = (end - beg + TRIP - 1) / TRIP;

  // A load's address is a wave-uniform row base (scalar registers) plus a 32-bit lane offset in bytes: the lane's column, and
  // one row stride for the odd row of the pair (h = 1).  A column past the edge is read from the last valid one: it feeds
  // output rows / columns that are never stored.  Rows at or past `end` are zeros in both operands: they are read from the last
  // row of the matrix (base clamped, the odd lanes' row step dropped) and replaced after the load, so the loads of a trip stay
  // unconditional and in flight together.
  uint32_t ca[TA], cb[2];
#pragma unroll
  for (int t = 0; t < TA; ++t) ca[t] = static_cast<uint32_t>(4 * (min(n0 + 32 * t + r, p.N - 1) * p.sdy1));
#pragma unroll
  for (int t = 0; t < 2; ++t) cb[t] = static_cast<uint32_t>(4 * min(k0 + 32 * t + r, p.K - 1));
  const uint32_t ha = static_cast<uint32_t>(4 * h * p.sdy0), hb = static_cast<uint32_t>(4 * h * p.sx0);

  auto load = [&](int64_t m0, float (&a)[TA][8], float (&b)[2][8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t row = m0 + 2 * e;                               // (wave-uniform)
      const int64_t rc = row < p.rows ? row : p.rows - 1;
      const char* ra = reinterpret_cast<const char*>(p.dy + rc * p.sdy0);
      const char* rb = reinterpret_cast<const char*>(p.x + rc * p.sx0);
      const bool ok = row + h < end;                                // end <= rows: the lane's row exists
#pragma unroll
      for (int t = 0; t < TA; ++t) {
        const float v = *reinterpret_cast<const float*>(ra + (ok ? ca[t] + ha : ca[t]));
        a[t][e] = ok ? v : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float v = *reinterpret_cast<const float*>(rb + (ok ? cb[t] + hb : cb[t]));
        b[t][e] = ok ? v : 0.f;
      }
    }
  };

  f32x16 acc[TA][2];
#pragma unroll
  for (int t = 0; t < TA; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[t][u][q] = 0.f;
  float asum[TA];
#pragma unroll
  for (int t = 0; t < TA; ++t) asum[t] = 0.f;

  auto mfmas = [&](const float (&a)[TA][8], const float (&b)[2][8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int t = 0; t < TA; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][e], b[u][e], acc[t][u], 0, 0, 0);
    if (want_db) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int t = 0; t < TA; ++t) asum[t] += a[t][e];
    }
  };

  // two operand buffers in turn: the next trip's loads are issued before this trip's MFMAs and fly under them.  A trip past the
  // slice loads nothing new (all zeros): at most one such trip per wave.
  float a0[TA][8], b0[2][8], a1[TA][8], b1[2][8];
  load(beg + TRIP * static_cast<int64_t>(wave), a0, b0);
  for (int64_t trip = wave; trip < ntrips; trip += 8) {
    load(beg + TRIP * (trip + 4), a1, b1);
    mfmas(a0, b0);
    load(beg + TRIP * (trip + 8), a0, b0);
    mfmas(a1, b1);
  }

  float* out = p.out + split * p.slab;
  if (want_db) {
#pragma unroll
    for (int t = 0; t < TA; ++t) asum_s[wave][t][lane] = asum[t];
  }
  // the four waves' partial tiles, one 32 x 32 tile at a time: wave w finishes accumulator registers 4w .. 4w+3 (rows
  // (q & 3) + 8 (q >> 2) + 4 h of the tile), in the fixed order (0 + 1) + (2 + 3)
#pragma unroll
  for (int t = 0; t < TA; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (t + u) __syncthreads();
#pragma unroll
      for (int q = 0; q < 16; ++q) red[wave][q][lane] = acc[t][u][q];
      __syncthreads();
      const int k = k0 + 32 * u + r;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int q = 4 * wave + s;
        const int n = n0 + 32 * t + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (n < p.N && k < p.K) {
          float v = (red[0][q][lane] + red[1][q][lane]) + (red[2][q][lane] + red[3][q][lane]);
          float* c = out + static_cast<int64_t>(n) * p.ldo + k;
          if (p.accumulate) v += *c;
          *c = v;
        }
      }
    }
  // column sums of dy: the two row parities of each wave, waves 0..3, one thread per column of the tile
  if (want_db && threadIdx.x < 32 * TA) {
    const int t = threadIdx.x >> 5, c = threadIdx.x & 31;
    const int n = n0 + 32 * t + c;
    if (n < p.N) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += asum_s[w][t][c] + asum_s[w][t][c + 32];
      p.db[split * p.db_slab + n] = s;
    }
  }
}

// dW[n, k] (+)= sum over the slabs in split order; db[n] = the same over the db slabs.  One thread per element.
__global__ void __launch_bounds__(256)
wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int N, int K, float* __restrict__ dW, int64_t ldw, int accumulate,
                    const float* __restrict__ ws_db, float* __restrict__ db) {
  const int nk = N * K;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < nk) {
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < splits; ++i) s += ws[static_cast<int64_t>(i) * nk + idx];
    float* c = dW + static_cast<int64_t>(idx / K) * ldw + idx % K;
    if (accumulate) s += *c;
    *c = s;
  } else if (db != nullptr && idx < nk + N) {
    const int n = idx - nk;
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < splits; ++i) s += ws_db[static_cast<int64_t>(i) * N + n];
    db[n] = s;
  }
}

inline bool wgrad_shape_ok(int64_t rows, int N, int K) {
  return rows >= 1 && rows < (static_cast<int64_t>(1) << 31) && N >= 1 && K >= 1 && N <= 512 && K <= 512;
}

}  // namespace

extern "C" {

int ns_gemm_wgrad_splits(int64_t rows, int N, int K) {
  if (!wgrad_shape_ok(rows, N, K)) return 1;
  return wgrad_shape(rows, N, K).splits;
}

int64_t ns_gemm_wgrad_workspace_bytes(int64_t rows, int N, int K) {
  if (!wgrad_shape_ok(rows, N, K)) return 0;
  const int splits = wgrad_shape(rows, N, K).splits;
  if (splits == 1) return 0;
  const int64_t bytes = static_cast<int64_t>(splits) * (static_cast<int64_t>(N) * K + N) * 4;
  return (bytes + 255) / 256 * 256;
}

int ns_gemm_wgrad(const float* dy_dev, int64_t dy_row_stride, int64_t dy_col_stride, const float* x_dev,
                  int64_t x_row_stride, int64_t rows, int N, int K, float* dW_dev, int64_t ldw, int accumulate,
                  float* db_dev, void* workspace_dev, void* stream) {
  NS_REQUIRE(rows >= 1 && rows < (static_cast<int64_t>(1) << 31), "rows must be in [1, 2^31)");
  NS_REQUIRE(N >= 1 && K >= 1, "bad shape");
  if (N > 512 || K > 512) {
    ns::set_error("%s: N and K are limited to 512 (got %d x %d)", __func__, N, K);
    return NS_E_UNSUPPORTED;
  }
  NS_REQUIRE(dy_dev && x_dev && dW_dev, "null pointer");
  NS_REQUIRE(dy_row_stride >= 0 && dy_col_stride >= 0 && x_row_stride >= 0 && ldw >= K, "bad stride");
  // a lane's offset inside a pair of rows is kept in 32 bits
  NS_REQUIRE(dy_row_stride < (1 << 28) && dy_col_stride < (1 << 19) && x_row_stride < (1 << 28), "stride too large");
  NS_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate is 0 or 1");
  const WgradShape s = wgrad_shape(rows, N, K);
  NS_REQUIRE(s.splits == 1 || workspace_dev, "this shape is split over workgroups and needs ns_gemm_wgrad_workspace_bytes of workspace");
  hipStream_t st = ns::as_stream(stream);
  WgradArgs a{};
  a.dy = dy_dev, a.sdy0 = dy_row_stride, a.sdy1 = dy_col_stride;
  a.x = x_dev, a.sx0 = x_row_stride;
  a.rows = rows, a.chunk = s.chunk;
  a.N = N, a.K = K, a.tiles_k = s.tiles_k;
  float* ws = static_cast<float*>(workspace_dev);
  float* ws_db = nullptr;
  if (s.splits == 1) {
    a.out = dW_dev, a.ldo = ldw, a.slab = 0, a.accumulate = accumulate;
    a.db = db_dev, a.db_slab = 0;
  } else {
    const int64_t nk = static_cast<int64_t>(N) * K;
    ws_db = ws + s.splits * nk;
    a.out = ws, a.ldo = K, a.slab = nk, a.accumulate = 0;
    a.db = db_dev ? ws_db : nullptr, a.db_slab = N;
  }
  const dim3 grid(s.tiles_n * s.tiles_k, s.splits);
  if (N <= 32) wgrad_kernel<1><<<grid, 256, 0, st>>>(a);
  else wgrad_kernel<2><<<grid, 256, 0, st>>>(a);
  NS_LAUNCH_CHECK();
  if (s.splits > 1) {
    const int total = N * K + (db_dev ? N : 0);
    wgrad_reduce_kernel<<<(total + 255) / 256, 256, 0, st>>>(ws, s.splits, N, K, dW_dev, ldw, accumulate, ws_db, db_dev);
    NS_LAUNCH_CHECK();
  }
  return NS_OK;
}

}  // extern "C"
