// The connected components of a mesh's faces on the device (ns_mesh_components): a lock-free union-find over the vertices, in the
// manner of ECL-CC (Jaiganesh and Burtscher, HPDC 2018).  Integers only; the result is a function of the inputs alone.
//
// parent[] IS label_dev.  Two invariants hold from the first launch to the last, whatever the order of the atomics:
//   (I1) parent[x] <= x, and parent[x] == x iff x is a root: a walk x -> parent[x] visits strictly decreasing indices, so it ends
//        after at most x steps, at a root that is the smallest index of its tree;
//   (I2) parent[x] lies in x's true component, and a word only ever decreases: it is written by the init store (x), by the hook
//        (atomicCAS root -> a smaller vertex of a face-connected tree) and by path halving (atomicMin with an ancestor).  The
//        hook merges two trees and halving keeps x in its tree: trees merge, they never split.
// Four launches on one stream, the kernel boundaries being the only synchronisation -- no workgroup waits for another's memory:
//   init     parent[v] = v, both counts 0, the two workspace counters 0;
//   hook     workgroup g takes faces [g * kShare, (g + 1) * kShare): a face out of range is counted and joins nothing, any other
//            unites (a, b) and (a, c) (unite: two walks side by side, path halving, a CAS on the larger root's own word);
//   flatten  label[v] = the root of v; the vertices are added per root and the roots counted, summed over the wave or the
//            workgroup first (block_add_by_key);
//   faces    a valid face adds 1 at the label of its first vertex, summed the same way; thread 0 writes the two totals as int64.
// VISIBILITY inside hook: every read of parent[] is a relaxed agent-scope atomic load (it bypasses the CU's L1), and every write
// an agent-scope read-modify-write.  Were a read stale all the same, it would return an OLDER value of the word: by (I2) a vertex
// of the same tree at or below x, from which the walk still ends at a root of x's tree -- a stale read costs steps, or one more
// turn of unite's loop, never a wrong hook or a wrong "they meet": whether r is still a root is decided by the atomicCAS on r's
// own word alone, and two positions that were ever in one tree still are.
#include "ns_block.h"
#include "ns_common.h"

namespace {

using ns::kBlock;
using ns::kWaves;
constexpr int kShare = NS_MESH_COMPONENTS_SHARE;
constexpr int kSteps = ns::ShareOf<kShare>::steps;

__device__ __forceinline__ int32_t load_word(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// joins the trees of a and b.  a and b are the positions of two walks towards the roots, ancestors-or-self of the two vertices;
// the two walks advance together, so their loads are in flight together, and the union is over as soon as they meet: two
// positions on one node, or below one parent, lie in one tree, and trees merge but never split (I2).  Most unions of a surface
// end there -- a vertex lies in six faces and needs one hook.
__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
  // terminates: a turn either returns, or replaces the larger root by old < hi after a CAS that failed because another thread's
  // hook of hi succeeded, or moves a to ga <= pa <= a and b to gb <= pb <= b with pa < a or pb < b (I1): a + b strictly
  // decreases every turn and is never below 0
  while (a != b) {
    const int32_t pa = load_word(parent + a), pb = load_word(parent + b);
    if (pa == a && pb == b) {                           // both read as roots: the CAS on hi's own word decides whether hi still is
      const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
      const int32_t old = atomicCAS(parent + hi, hi, lo);
      if (old == hi) return;                            // hi was a root and now hangs below lo < hi
      a = old;
      b = lo;                                           // perhaps no root any more: a root may hang below any smaller vertex
      continue;
    }
    if (pa == pb) return;
    const int32_t ga = load_word(parent + pa), gb = load_word(parent + pb);
    if (ga != pa) atomicMin(parent + a, ga);            // path halving: ga is an ancestor of a below pa, so (I1) and (I2) hold;
    if (gb != pb) atomicMin(parent + b, gb);            // no value is returned, nobody waits for it
    a = ga;
    b = gb;
  }
}

// the three indices of face e; true iff all lie in [0, V)
__device__ __forceinline__ bool face_load(const int64_t* __restrict__ faces, int64_t e, int64_t V, int32_t (&v)[3]) {
  const int64_t a = faces[e * 3], b = faces[e * 3 + 1], c = faces[e * 3 + 2];
  const bool ok = a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
  v[0] = static_cast<int32_t>(a), v[1] = static_cast<int32_t>(b), v[2] = static_cast<int32_t>(c);   // used only where ok
  return ok;
}

// counts[key] += the number of active lanes of this wave with that key: one atomic per distinct key.  Every lane of the wave calls.
__device__ __forceinline__ void wave_add_by_key(int32_t* counts, int32_t key, bool active) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(active);
  // terminates: every turn retires at least the leader's lane from todo, so at most 64 turns
  while (todo != 0ull) {
    const int leader = __ffsll(static_cast<long long>(todo)) - 1;
    const int32_t k = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(active && key == k);
    if (lane == leader) atomicAdd(counts + k, static_cast<int32_t>(__popcll(same)));
    todo &= ~same;
  }
}

// counts[key[s]] += 1 for every active item of the workgroup.  A surface is mostly one component: the items that carry the key of
// the workgroup's first item are summed over the workgroup and added once -- per wave they would queue 16 atomics per workgroup
// on ONE word --, the others per wave.  Every thread of the workgroup calls.
__device__ __forceinline__ void block_add_by_key(int32_t* counts, const int32_t (&key)[kSteps], const bool (&active)[kSteps],
                                                 int* wave_sums, int* first_key) {
  if (threadIdx.x == 0) *first_key = active[0] ? key[0] : -1;                  // -1: no item carries it
  __syncthreads();
  const int32_t k0 = *first_key;
  int mine = 0;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const bool first = active[s] && key[s] == k0;
    mine += first ? 1 : 0;
    wave_add_by_key(counts, key[s], active[s] && !first);
  }
  const int total = ns::block_sum(mine, wave_sums);
  if (threadIdx.x == 0 && total != 0) atomicAdd(counts + k0, total);
}

// counters[0] = ignored faces, counters[1] = components
__global__ void __launch_bounds__(kBlock)
cc_init_kernel(int32_t* __restrict__ parent, int32_t* __restrict__ tri_count, int32_t* __restrict__ vert_count, int64_t V,
               int32_t* __restrict__ counters) {
  if (blockIdx.x == 0 && threadIdx.x < 2) counters[threadIdx.x] = 0;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t v = base + s * kBlock;
    if (v < V) {
      parent[v] = static_cast<int32_t>(v);
      tri_count[v] = 0;
      vert_count[v] = 0;
    }
  }
}

__global__ void __launch_bounds__(kBlock)
cc_hook_kernel(const int64_t* __restrict__ faces, int64_t F, int64_t V, int32_t* parent, int32_t* counters) {
  __shared__ int wave_sums[kWaves];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
  int ignored = 0;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t e = base + s * kBlock;
    if (e >= F) continue;
    int32_t v[3];
    if (!face_load(faces, e, V, v)) {
      ++ignored;
      continue;
    }
    if (v[0] != v[1]) unite(parent, v[0], v[1]);
    if (v[0] != v[2] && v[1] != v[2]) unite(parent, v[0], v[2]);
  }
  const int total = ns::block_sum(ignored, wave_sums);
  if (threadIdx.x == 0 && total != 0) atomicAdd(counters, total);
}

__global__ void __launch_bounds__(kBlock)
cc_flatten_kernel(int32_t* label, int32_t* vert_count, int64_t V, int32_t* counters) {
  __shared__ int wave_sums[2][kWaves];
  __shared__ int first_key;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
  int roots = 0;
  int32_t root[kSteps];
  bool active[kSteps];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t v = base + s * kBlock;
    active[s] = v < V;
    int32_t r = 0;
    if (active[s]) {
      // a word read here is either what hook left or the root another thread of this launch stored: both are ancestors of v
      // at or below it.  Terminates: r strictly decreases until label[r] == r (I1), and a root's word is never written here
      // with anything but itself
      r = static_cast<int32_t>(v);
      for (int32_t p = load_word(label + r); p != r; p = load_word(label + r)) r = p;
      __hip_atomic_store(label + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      roots += r == static_cast<int32_t>(v) ? 1 : 0;
    }
    root[s] = r;
  }
  block_add_by_key(vert_count, root, active, wave_sums[0], &first_key);
  const int total = ns::block_sum(roots, wave_sums[1]);
  if (threadIdx.x == 0 && total != 0) atomicAdd(counters + 1, total);
}

__global__ void __launch_bounds__(kBlock)
cc_faces_kernel(const int64_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ label,
                int32_t* tri_count, const int32_t* __restrict__ counters, int64_t* __restrict__ count_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {            // both counters are complete: their launches lie before this one
    count_out[0] = counters[1];
    count_out[1] = counters[0];
  }
  __shared__ int wave_sums[kWaves];
  __shared__ int first_key;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
  int32_t root[kSteps];
  bool active[kSteps];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t e = base + s * kBlock;
    int32_t v[3];
    active[s] = e < F && face_load(faces, e, V, v);
    root[s] = active[s] ? label[v[0]] : 0;
  }
  block_add_by_key(tri_count, root, active, wave_sums, &first_key);
}

// V == 0: there is no vertex, so every face is out of range
__global__ void cc_empty_kernel(int64_t* __restrict__ count_out, int64_t F) {
  count_out[0] = 0;
  count_out[1] = F;
}

bool cc_shape_ok(int64_t V, int64_t F) { return V >= 0 && F >= 0 && ns::below_2_31(V) && ns::below_2_31(F); }

}  // namespace

extern "C" {

int64_t ns_mesh_components_workspace_bytes(int64_t V, int64_t F) { return cc_shape_ok(V, F) ? 256 : 0; }

int ns_mesh_components(const int64_t* faces_dev, int64_t F, int64_t V, int32_t* label_dev, int32_t* tri_count_dev,
                       int32_t* vert_count_dev, int64_t* count_dev, void* workspace_dev, void* stream) {
  NS_REQUIRE(F >= 0 && V >= 0, "negative F or V");
  NS_REQUIRE(cc_shape_ok(V, F), "V and F must be below 2^31");
  NS_REQUIRE(count_dev, "count_dev is required");
  NS_REQUIRE(F == 0 || faces_dev, "faces_dev is required when F > 0");
  NS_REQUIRE(V == 0 || (label_dev && tri_count_dev && vert_count_dev && workspace_dev),
             "label_dev, tri_count_dev, vert_count_dev and workspace_dev are required when V > 0");
  NS_REQUIRE(ns::aligned(count_dev, 8) && ns::aligned(workspace_dev, 8) && ns::aligned(faces_dev, 8),
             "count_dev, workspace_dev and faces_dev are 8-byte aligned");
  NS_REQUIRE(ns::aligned(label_dev, 4) && ns::aligned(tri_count_dev, 4) && ns::aligned(vert_count_dev, 4),
             "label_dev, tri_count_dev and vert_count_dev are 4-byte aligned");
  hipStream_t s = ns::as_stream(stream);
  if (V == 0) {
    cc_empty_kernel<<<1, 1, 0, s>>>(count_dev, F);
    NS_LAUNCH_CHECK();
    return NS_OK;
  }
  int32_t* counters = static_cast<int32_t*>(workspace_dev);
  const int v_groups = static_cast<int>(ns::cdiv(V, kShare));                       // at most 2^31 / NS_MESH_COMPONENTS_SHARE
  const int f_groups = static_cast<int>(ns::cdiv(F, kShare));
  cc_init_kernel<<<v_groups, kBlock, 0, s>>>(label_dev, tri_count_dev, vert_count_dev, V, counters);
  NS_LAUNCH_CHECK();
  if (f_groups > 0) {
    cc_hook_kernel<<<f_groups, kBlock, 0, s>>>(faces_dev, F, V, label_dev, counters);
    NS_LAUNCH_CHECK();
  }
  cc_flatten_kernel<<<v_groups, kBlock, 0, s>>>(label_dev, vert_count_dev, V, counters);
  NS_LAUNCH_CHECK();
  cc_faces_kernel<<<f_groups > 0 ? f_groups : 1, kBlock, 0, s>>>(faces_dev, F, V, label_dev, tri_count_dev, counters, count_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // extern "C"
