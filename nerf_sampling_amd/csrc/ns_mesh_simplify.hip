// A mesh simplified by vertex clustering on the device (ns_mesh_simplify): Rossignac and Borrel's clustering on a coarse lattice,
// with a cluster represented by ONE OF ITS OWN vertices -- the member nearest the cluster's centroid -- so every vertex that stays
// is an input vertex, bit for bit.  The definitions (fixed-point coordinate, cell, distance) are ns_mesh_cluster.h's; built with
// -ffp-contract=off, every fp64 operation rounded on its own.  The result is a function of the inputs alone:
//   accumulate  integer atomicAdd of u (int64, three sums) and of 1 (int32) per member: S < 2^31 * 2^31, no overflow, any order;
//   choose      the member with the smallest word (bits((float) d) << 32) | v, merged by a 64-bit unsigned atomicMin as the
//               rasteriser's z-buffer is: d >= 0, so the bits order as the values do, and ties go to the smaller index;
//   faces       an ordered stream compaction without atomics (ns_block.h: per-share counts, share_scan, share_place).
// Seven launches on one stream, the kernel boundaries being the only synchronisation, nothing read back in between:
//   clear       the table (sums and counts 0, words all ones) and the two 32-bit counters;
//   accumulate  workgroup g takes vertices [g * kShare, (g + 1) * kShare); non-finite vertices are counted;
//   choose      every member reads its cluster's finished sums and offers its word;
//   resolve     rep[v] = the low half of its cluster's word (-1 for a non-finite vertex); representatives are counted;
//   count       workgroup g classifies faces [g * kShare, (g + 1) * kShare): kept, collapsed, invalid, on a non-finite vertex;
//   scan        ONE workgroup turns the kept counts into output indices and writes the six totals;
//   emit        every workgroup classifies its faces again and writes the kept ones at index + earlier (step, wave) groups + lanes
//               below, in input order, windings kept; what lies at or beyond the capacity is not written.
// A face is judged in this order: an index outside [0, V) -> invalid (none of its indices is used as an address); else a corner
// with rep == -1 -> on a non-finite vertex; else two equal representatives -> collapsed; else kept.
#include <cmath>

#include "ns_block.h"
#include "ns_common.h"
#include "ns_mesh_cluster.h"

namespace {

using ns::kBlock;
using ns::kWaves;
using ns_cluster::Lattice;
constexpr int kShare = NS_MESH_SIMPLIFY_SHARE;
constexpr int kSteps = ns::ShareOf<kShare>::steps;
constexpr unsigned long long kEmpty = ~0ull;

struct alignas(8) Cluster {                 // 40 bytes = five 64-bit words; word 3 is the representative's
  unsigned long long S[3];                  // the sums of u: below 2^62
  unsigned long long word;
  int32_t n;
  int32_t pad;
};
static_assert(sizeof(Cluster) == 40, "five words per cluster");
constexpr int kClusterWords = 5, kWordSlot = 3;

enum Verdict { kKept = 0, kCollapsed = 1, kInvalid = 2, kOnNonfinite = 3 };

// vertex v < V: its coordinate and cell; false for a non-finite one
__device__ __forceinline__ bool vertex_load(const Lattice& L, const float* __restrict__ vertices, int64_t v, int32_t (&u)[3],
                                            int32_t& cell) {
  const float p[3] = {vertices[v * 3], vertices[v * 3 + 1], vertices[v * 3 + 2]};
  const bool ok = ns_cluster::vertex_coord(L, p, u);
  cell = ns_cluster::cell_index(L, u);                                         // 0 where !ok: never used then
  return ok;
}

// words: the table as 64-bit words; counters[0] = non-finite vertices, counters[1] = representatives
__global__ void __launch_bounds__(kBlock)
simplify_clear_kernel(unsigned long long* __restrict__ words, int64_t n_words, int32_t* __restrict__ counters) {
  if (blockIdx.x == 0 && threadIdx.x < 2) counters[threadIdx.x] = 0;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t w = base + s * kBlock;
    if (w < n_words) words[w] = (w % kClusterWords == kWordSlot) ? kEmpty : 0ull;
  }
}

__global__ void __launch_bounds__(kBlock)
simplify_accumulate_kernel(Lattice L, const float* __restrict__ vertices, int64_t V, Cluster* table, int32_t* counters) {
  __shared__ int wave_sums[kWaves];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
  int nonfinite = 0;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t v = base + s * kBlock;
    if (v >= V) continue;
    int32_t u[3], cell;
    if (!vertex_load(L, vertices, v, u, cell)) {
      ++nonfinite;
      continue;
    }
    Cluster* c = table + cell;
    atomicAdd(&c->S[0], static_cast<unsigned long long>(u[0]));                // u >= 0
    atomicAdd(&c->S[1], static_cast<unsigned long long>(u[1]));
    atomicAdd(&c->S[2], static_cast<unsigned long long>(u[2]));
    atomicAdd(&c->n, 1);
  }
  const int total = ns::block_sum(nonfinite, wave_sums);
  if (threadIdx.x == 0 && total != 0) atomicAdd(counters, total);
}

__global__ void __launch_bounds__(kBlock)
simplify_choose_kernel(Lattice L, const float* __restrict__ vertices, int64_t V, Cluster* table) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t v = base + s * kBlock;
    if (v >= V) continue;
    int32_t u[3], cell;
    if (!vertex_load(L, vertices, v, u, cell)) continue;
    Cluster* c = table + cell;                                                 // its sums are complete: their launch lies before
    const int64_t S[3] = {static_cast<int64_t>(c->S[0]), static_cast<int64_t>(c->S[1]), static_cast<int64_t>(c->S[2])};
    const float d32 = ns_cluster::distance2(u, S, c->n);                       // n >= 1: v itself is a member
    atomicMin(&c->word, (static_cast<unsigned long long>(__float_as_uint(d32)) << 32) | static_cast<uint32_t>(v));
  }
}

__global__ void __launch_bounds__(kBlock)
simplify_resolve_kernel(Lattice L, const float* __restrict__ vertices, int64_t V, const Cluster* __restrict__ table,
                        int32_t* __restrict__ rep_out, int32_t* counters) {
  __shared__ int wave_sums[kWaves];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
  int reps = 0;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t v = base + s * kBlock;
    if (v >= V) continue;
    int32_t u[3], cell, rep = -1;
    if (vertex_load(L, vertices, v, u, cell)) rep = static_cast<int32_t>(table[cell].word & 0xffffffffull);   // a member: below V
    rep_out[v] = rep;
    reps += rep == static_cast<int32_t>(v) ? 1 : 0;
  }
  const int total = ns::block_sum(reps, wave_sums);
  if (threadIdx.x == 0 && total != 0) atomicAdd(counters + 1, total);
}

// the verdict on face e < F and, where it is kept, its three representatives
__device__ __forceinline__ Verdict face_map(const int64_t* __restrict__ faces, int64_t e, int64_t V,
                                            const int32_t* __restrict__ rep, int32_t (&r)[3]) {
  const int64_t a = faces[e * 3], b = faces[e * 3 + 1], c = faces[e * 3 + 2];
  if (!(a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V)) return kInvalid;
  r[0] = rep[a], r[1] = rep[b], r[2] = rep[c];
  if (r[0] < 0 || r[1] < 0 || r[2] < 0) return kOnNonfinite;
  if (r[0] == r[1] || r[0] == r[2] || r[1] == r[2]) return kCollapsed;
  return kKept;
}

// counts[k * groups + g] = the faces of share g with verdict k, k = 0 .. 3
__global__ void __launch_bounds__(kBlock)
simplify_count_kernel(const int64_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ rep,
                      int64_t* __restrict__ counts, int groups) {
  __shared__ int wave_counts[4][kWaves];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
  int n[4] = {0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t e = base + s * kBlock;
    if (e >= F) continue;
    int32_t r[3];
    const Verdict k = face_map(faces, e, V, rep, r);
#pragma unroll
    for (int q = 0; q < 4; ++q) n[q] += k == q ? 1 : 0;
  }
  ns::wave_sum_to(n[0], wave_counts[0], n[1], wave_counts[1]);
  ns::wave_sum_to(n[2], wave_counts[2], n[3], wave_counts[3]);
  __syncthreads();                                         // one barrier for the four sums
  if (threadIdx.x < 4) counts[static_cast<int64_t>(threadIdx.x) * groups + blockIdx.x] = ns::slots_sum(wave_counts[threadIdx.x]);
}

// counts[g] <- counts[0] + ... + counts[g - 1] (ns::share_scan, one workgroup; groups == 0: nothing to scan); the totals:
// totals[0] kept faces, [1] collapsed, [2] invalid, [3] non-finite vertices, [4] faces on one, [5] representatives
__global__ void __launch_bounds__(kBlock)
simplify_scan_kernel(int64_t* __restrict__ counts, int groups, const int32_t* __restrict__ counters, int64_t* __restrict__ totals) {
  __shared__ int64_t wave_extra[3][kWaves];
  int64_t extra[3] = {0, 0, 0};
  const int64_t kept = ns::share_scan(counts, groups, 0, [&](int g, bool in_range) {
#pragma unroll
    for (int q = 0; q < 3; ++q) extra[q] += in_range ? counts[static_cast<int64_t>(q + 1) * groups + g] : 0;
  });
  ns::wave_sum_to(extra[0], wave_extra[0], extra[1], wave_extra[1]);
  ns::wave_sum_to(extra[2], wave_extra[2]);
  __syncthreads();
  if (threadIdx.x == 0) {
    totals[0] = kept;
    totals[1] = ns::slots_sum(wave_extra[0]);
    totals[2] = ns::slots_sum(wave_extra[1]);
    totals[3] = counters[0];                               // both are complete: their launches lie before this one
    totals[4] = ns::slots_sum(wave_extra[2]);
    totals[5] = counters[1];
  }
}

__global__ void __launch_bounds__(kBlock)
simplify_emit_kernel(const int64_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ rep,
                     const int64_t* __restrict__ bases, int64_t* __restrict__ faces_out, int64_t capacity) {
  __shared__ int cell_counts[kSteps][kWaves];
  const int64_t first = bases[blockIdx.x];
  if (first >= capacity) return;                           // every face of this share lies at or beyond the capacity
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
  int32_t r[kSteps][3];
  bool kept[kSteps];
  ns::share_place<kSteps>(
      [&](int s) {
        const int64_t e = base + s * kBlock;
        kept[s] = e < F && face_map(faces, e, V, rep, r[s]) == kKept;
        return kept[s];
      },
      cell_counts,
      [&](int s, int at) {
        const int64_t n = first + at;
        if (!kept[s] || n >= capacity) return;             // beyond the capacity: counted by the scan, never written
        faces_out[n * 3] = r[s][0];
        faces_out[n * 3 + 1] = r[s][1];
        faces_out[n * 3 + 2] = r[s][2];
      });
}

bool count_ok(int64_t n) { return n >= 0 && ns::below_2_31(n); }

bool dims_ok(int Cx, int Cy, int Cz) {
  const Lattice L{{0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}, {Cx, Cy, Cz}};
  return ns_cluster::lattice_ok(L);
}

// the workspace: 256 bytes of counters, the four per-share face counts, the table
int64_t counts_bytes(int64_t F) { return ns::round_256(ns::cdiv(F, kShare) * 4 * static_cast<int64_t>(sizeof(int64_t))); }
int64_t table_bytes(int Cx, int Cy, int Cz) {
  return ns::round_256(static_cast<int64_t>(Cx) * Cy * Cz * static_cast<int64_t>(sizeof(Cluster)));
}

}  // namespace

extern "C" {

int64_t ns_mesh_simplify_workspace_bytes(int64_t V, int64_t F, int Cx, int Cy, int Cz) {
  if (!count_ok(V) || !count_ok(F) || !dims_ok(Cx, Cy, Cz)) return 0;
  return 256 + counts_bytes(F) + table_bytes(Cx, Cy, Cz);
}

int ns_mesh_cluster_coord(const float* vertex_host, const float* lo_host, const float* cell_host, const int* dims_host,
                          int32_t* u_out, int32_t* cell_out) {
  NS_REQUIRE(vertex_host && lo_host && cell_host && dims_host && u_out && cell_out, "null pointer");
  Lattice L;
  for (int x = 0; x < 3; ++x) L.lo[x] = lo_host[x], L.cell[x] = cell_host[x], L.C[x] = dims_host[x];
  NS_REQUIRE(ns_cluster::lattice_ok(L), "lo finite, cell finite and positive, dims in [1, 2^15] with a product of at most 2^24");
  const float p[3] = {vertex_host[0], vertex_host[1], vertex_host[2]};
  int32_t u[3];
  const bool ok = ns_cluster::vertex_coord(L, p, u);
  for (int x = 0; x < 3; ++x) u_out[x] = u[x];
  *cell_out = ok ? ns_cluster::cell_index(L, u) : -1;
  return ok ? 1 : 0;
}

int ns_mesh_cluster_distance(const int32_t* u_host, const int64_t* sums_host, int32_t n, float* d_out) {
  NS_REQUIRE(u_host && sums_host && d_out, "null pointer");
  NS_REQUIRE(n >= 1, "n must be at least 1");
  const int32_t u[3] = {u_host[0], u_host[1], u_host[2]};
  const int64_t S[3] = {sums_host[0], sums_host[1], sums_host[2]};
  *d_out = ns_cluster::distance2(u, S, n);
  return NS_OK;
}

int ns_mesh_simplify(const float* vertices_dev, int64_t V, const int64_t* faces_dev, int64_t F, const float* lo_host,
                     const float* cell_host, const int* dims_host, int32_t* rep_out, int64_t* faces_out, int64_t capacity,
                     int64_t* count_dev, void* workspace_dev, void* stream) {
  NS_REQUIRE(count_ok(V) && count_ok(F), "V and F must lie in [0, 2^31)");
  NS_REQUIRE(lo_host && cell_host && dims_host, "lo_host, cell_host and dims_host are required");
  Lattice L;
  for (int x = 0; x < 3; ++x) L.lo[x] = lo_host[x], L.cell[x] = cell_host[x], L.C[x] = dims_host[x];
  NS_REQUIRE(ns_cluster::lattice_ok(L), "lo finite, cell finite and positive, dims in [1, 2^15] with a product of at most 2^24");
  NS_REQUIRE(capacity >= 0, "negative capacity");
  NS_REQUIRE(count_dev && workspace_dev, "count_dev and workspace_dev are required");
  NS_REQUIRE(V == 0 || (vertices_dev && rep_out), "vertices_dev and rep_out are required when V > 0");
  NS_REQUIRE(F == 0 || faces_dev, "faces_dev is required when F > 0");
  NS_REQUIRE(F == 0 || capacity == 0 || faces_out, "faces_out is required when F > 0 and capacity > 0");
  NS_REQUIRE(ns::aligned(faces_dev, 8) && ns::aligned(faces_out, 8) && ns::aligned(count_dev, 8) && ns::aligned(workspace_dev, 8),
             "faces_dev, faces_out, count_dev and workspace_dev are 8-byte aligned");
  NS_REQUIRE(ns::aligned(vertices_dev, 4) && ns::aligned(rep_out, 4), "vertices_dev and rep_out are 4-byte aligned");
  char* ws = static_cast<char*>(workspace_dev);
  int32_t* counters = reinterpret_cast<int32_t*>(ws);
  int64_t* counts = reinterpret_cast<int64_t*>(ws + 256);
  Cluster* table = reinterpret_cast<Cluster*>(ws + 256 + counts_bytes(F));
  const int64_t n_words = static_cast<int64_t>(L.C[0]) * L.C[1] * L.C[2] * kClusterWords;       // at most 5 * 2^24
  const int w_groups = static_cast<int>(ns::cdiv(n_words, kShare));
  const int v_groups = static_cast<int>(ns::cdiv(V, kShare));                 // at most 2^31 / NS_MESH_SIMPLIFY_SHARE
  const int f_groups = static_cast<int>(ns::cdiv(F, kShare));
  hipStream_t s = ns::as_stream(stream);
  simplify_clear_kernel<<<w_groups, kBlock, 0, s>>>(reinterpret_cast<unsigned long long*>(table), n_words, counters);
  NS_LAUNCH_CHECK();
  if (v_groups > 0) {
    simplify_accumulate_kernel<<<v_groups, kBlock, 0, s>>>(L, vertices_dev, V, table, counters);
    NS_LAUNCH_CHECK();
    simplify_choose_kernel<<<v_groups, kBlock, 0, s>>>(L, vertices_dev, V, table);
    NS_LAUNCH_CHECK();
    simplify_resolve_kernel<<<v_groups, kBlock, 0, s>>>(L, vertices_dev, V, table, rep_out, counters);
    NS_LAUNCH_CHECK();
  }
  if (f_groups > 0) {
    simplify_count_kernel<<<f_groups, kBlock, 0, s>>>(faces_dev, F, V, rep_out, counts, f_groups);
    NS_LAUNCH_CHECK();
  }
  simplify_scan_kernel<<<1, kBlock, 0, s>>>(counts, f_groups, counters, count_dev);
  NS_LAUNCH_CHECK();
  if (f_groups > 0 && capacity > 0) {
    simplify_emit_kernel<<<f_groups, kBlock, 0, s>>>(faces_dev, F, V, rep_out, counts, faces_out, capacity);
    NS_LAUNCH_CHECK();
  }
  return NS_OK;
}

}  // extern "C"
