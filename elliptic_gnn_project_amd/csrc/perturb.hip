// K15 — seeded input perturbations of the robustness analysis (src/analysis/robustness.py):
// uniform edge drop (drop_edges, :65-82) and Gaussian feature noise (maybe_add_noise, :85-90), from
// the counter hash of the dropout mask (gemm_common.hpp keep_elem) in place of torch's device RNG,
// so that a trial has a bit-exact host mirror (elliptic_gnn_project_amd/robustness.py).
//
//   H(c, key) = fmix32(((uint32)c * 0x9E3779B1 + key_lo) ^ key_hi)     a bijection on uint32
//
// Edge drop: the drop_count edges with the smallest (H(e, key), e) go; the others keep their order.
// hash -> one stable rocPRIM radix sort of (hash, edge id) -> keep flag per edge from its sorted
// position -> exclusive scan -> compaction of both rows.  The output size is the caller's
// E - drop_count: no host synchronisation, nothing a stream capture cannot record.
//
// Noise: one Box-Muller pair per two neighbouring columns of a row, counter c = row·ceil(F/2) + col/2:
//   u1 = ((H(c, key_r) >> 8) + 1)·2^-24 in (0, 1],  u2 = (H(c, key_a) >> 8)·2^-24 in [0, 1)
//   r = sqrt(-2 ln u1),  z_even = r·cos(2π u2),  z_odd = r·sin(2π u2),  out = x + noise_std·z
// with the precise logf / sqrtf / sincospif (2·u2 is exact, so is the reduction).  The two stream
// keys come from the call's key on the host: stream_key(key, 2) the radius', stream_key(key, 3) the angle's.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"
#include "edge_compact.hpp"

namespace gnnmp {
namespace {

constexpr int kTB = 256;

__host__ __device__ __forceinline__ uint32_t perturb_hash(uint32_t c, uint64_t key) {
  uint32_t h = c * 0x9E3779B1u + (uint32_t)key;
  h ^= (uint32_t)(key >> 32);
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// key(seed, stream) = splitmix64(seed ^ (stream * 0xD1B54A32D192ED03)), arithmetic mod 2^64
inline uint64_t stream_key(uint64_t seed, uint64_t stream) {
  uint64_t z = (seed ^ (stream * 0xD1B54A32D192ED03ull)) + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ------------------------------------------------------------------------ edge drop
__global__ void drop_hash_kernel(int64_t E, uint64_t key, uint32_t* __restrict__ hash, int32_t* __restrict__ eid) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= E) return;
  hash[e] = perturb_hash((uint32_t)e, key);
  eid[e] = (int32_t)e;
}

// sorted position t holds edge order[t]: the first drop_count positions are the dropped edges
__global__ void drop_flags_kernel(const int32_t* __restrict__ order, int64_t E, int64_t drop_count,
                                  int32_t* __restrict__ keep) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= E) return;
  keep[order[t]] = t >= drop_count ? 1 : 0;
}

struct DropLayout {
  uint32_t *hash, *hash_out;
  int32_t *eid, *order;
  void* tmp;
  size_t tmp_bytes;
  int32_t *keep, *pos;  // the sort's key buffers again (dead once the order is known)
};

gnn_status drop_tmp_bytes(int64_t E, size_t* bytes) {
  const size_t n = (size_t)(E > 0 ? E : 1);
  size_t sb = 0, tb = 0;
  hipError_t err = rocprim::radix_sort_pairs(nullptr, sb, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr,
                                             (int32_t*)nullptr, n, 0, 32, (hipStream_t)0);
  if (err != hipSuccess) return hip_check(err, "drop_tmp_bytes (sort)");
  gnn_status s = edge_compact_tmp_bytes(E, (const int32_t*)nullptr, &tb);
  if (s != GNN_OK) return s;
  *bytes = sb > tb ? sb : tb;
  return GNN_OK;
}

struct SizerAdapter {
  WorkspaceSizer s;
  template <typename T>
  T* take(size_t n) { s.take<T>(n); return nullptr; }
};

template <typename C>
void carve_drop(C& c, int64_t E, size_t tmp_bytes, DropLayout* L) {
  const size_t n = (size_t)(E > 0 ? E : 1);
  auto a = c.template take<uint32_t>(n);
  auto b = c.template take<uint32_t>(n);
  auto v = c.template take<int32_t>(n);
  auto o = c.template take<int32_t>(n);
  auto t = c.template take<char>(tmp_bytes);
  if (L) {
    L->hash = a; L->hash_out = b; L->eid = v; L->order = o; L->tmp = (void*)t; L->tmp_bytes = tmp_bytes;
    L->keep = (int32_t*)a; L->pos = (int32_t*)b;
  }
}

// ------------------------------------------------------------------------ feature noise
// The standard-normal pair of counter c.
__device__ __forceinline__ void noise_pair(uint32_t c, uint64_t key_r, uint64_t key_a, float* z0, float* z1) {
  const uint32_t a = perturb_hash(c, key_r) >> 8, b = perturb_hash(c, key_a) >> 8;
  const float u1 = (float)(a + 1u) * 0x1p-24f;  // exact: a + 1 <= 2^24
  const float t2 = (float)b * 0x1p-23f;         // 2·u2, exact
  const float r = sqrtf(-2.0f * logf(u1));
  float s, co;
  sincospif(t2, &s, &co);
  *z0 = r * co;
  *z1 = r * s;
}

// One thread per group of VEC columns of a row (VEC 4: two pairs, 16-byte accesses; VEC 2: one pair,
// 8-byte accesses; VEC 1: one pair, 4-byte accesses).  G groups per row; rows·G < 2^32 (the counter
// limit rows·ceil(F/2) < 2^32 covers it).  The row's last group may be partial: element by element.
template <int VEC>
__global__ __launch_bounds__(kTB) void noise_kernel(const float* __restrict__ x, int64_t ldx, uint32_t rows,
                                                    uint32_t F, uint32_t G, uint32_t P, float noise_std,
                                                    uint64_t key_r, uint64_t key_a, float* __restrict__ out,
                                                    int64_t ldo) {
  constexpr int W = VEC == 1 ? 2 : VEC;  // columns per thread
  const uint64_t t64 = blockIdx.x * (uint64_t)kTB + threadIdx.x;
  if (t64 >= (uint64_t)rows * G) return;
  const uint32_t t = (uint32_t)t64;
  const uint32_t row = t / G, g = t - row * G;
  const uint32_t c0 = g * W;  // first column, even
  const float* xr = x + (int64_t)row * ldx + c0;
  float* yr = out + (int64_t)row * ldo + c0;
  float z[W];
#pragma unroll
  for (int q = 0; q < W; q += 2) {
    if (c0 + q < F) noise_pair(row * P + ((c0 + q) >> 1), key_r, key_a, &z[q], &z[q + 1]);
    else z[q] = z[q + 1] = 0.f;
  }
  if constexpr (VEC > 1) {
    if (c0 + W <= F) {
      using V = typename std::conditional<VEC == 4, float4, float2>::type;
      V v = *reinterpret_cast<const V*>(xr);
      float* e = reinterpret_cast<float*>(&v);
#pragma unroll
      for (int q = 0; q < W; ++q) e[q] = e[q] + noise_std * z[q];
      *reinterpret_cast<V*>(yr) = v;
      return;
    }
  }
#pragma unroll
  for (int q = 0; q < W; ++q)
    if (c0 + q < F) yr[q] = xr[q] + noise_std * z[q];
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" gnn_status gnn_edge_drop_workspace_size(int64_t num_edges, size_t* bytes) {
  if (!bytes || num_edges < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  if (num_edges >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "num_edges exceeds int32 range");
  size_t tb = 0;
  gnn_status s = drop_tmp_bytes(num_edges, &tb);
  if (s != GNN_OK) return s;
  SizerAdapter a;
  carve_drop(a, num_edges, tb, nullptr);
  *bytes = a.s.used + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_edge_drop(const int64_t* edge_index, int64_t num_edges, int64_t drop_count, uint64_t key,
                                    int64_t* out, void* workspace, size_t workspace_bytes, gnn_stream_t stream) {
  const int64_t E = num_edges;
  if (E < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative num_edges");
  if (E >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "num_edges exceeds int32 range");
  if (E == 0) return drop_count == 0 ? GNN_OK : fail(GNN_ERR_INVALID_ARG, __func__, "drop_count outside [0, num_edges)");
  if (drop_count < 0 || drop_count >= E) return fail(GNN_ERR_INVALID_ARG, __func__, "drop_count outside [0, num_edges)");
  if (drop_count == 0) return GNN_OK;  // nothing dropped: the caller keeps edge_index itself
  if (!edge_index || !out) return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  hipStream_t st = (hipStream_t)stream;
  size_t tb = 0;
  gnn_status s = drop_tmp_bytes(E, &tb);
  if (s != GNN_OK) return s;
  WorkspaceCarver c(workspace, workspace_bytes);
  DropLayout L;
  carve_drop(c, E, tb, &L);
  if (!workspace || !c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  const unsigned nb = (unsigned)ceil_div(E, kTB);
  drop_hash_kernel<<<nb, kTB, 0, st>>>(E, key, L.hash, L.eid);
  GNN_LAUNCH_CHECK();
  size_t sb = L.tmp_bytes;
  GNN_HIP_TRY(rocprim::radix_sort_pairs(L.tmp, sb, L.hash, L.hash_out, L.eid, L.order, (size_t)E, 0, 32, st));
  drop_flags_kernel<<<nb, kTB, 0, st>>>(L.order, E, drop_count, L.keep);
  GNN_LAUNCH_CHECK();
  // exclusive scan of the flags and compaction of both rows (edge_compact.hpp, shared with hub.hip)
  return edge_compact(edge_index, E, E - drop_count, (const int32_t*)L.keep, KeepFlag{L.keep}, L.pos, L.tmp, L.tmp_bytes,
                      out, st);
}

extern "C" gnn_status gnn_feature_noise_f32(const float* x, int64_t ldx, int64_t rows, int64_t F, float noise_std,
                                            uint64_t key, float* out, int64_t ldo, gnn_stream_t stream) {
  if (rows < 0 || F < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative rows or F");
  if (rows == 0 || F == 0) return GNN_OK;
  if (!x || !out) return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  if (ldx < F || ldo < F) return fail(GNN_ERR_INVALID_ARG, __func__, "leading dimension below F");
  const int64_t P = (F + 1) / 2;
  if (rows > (int64_t)UINT32_MAX / P) return fail(GNN_ERR_INVALID_ARG, __func__, "rows * ceil(F/2) exceeds the 32-bit counter");
  const uint64_t key_radius = stream_key(key, 2), key_angle = stream_key(key, 3);
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  const bool v4 = xa % 16 == 0 && oa % 16 == 0 && ldx % 4 == 0 && ldo % 4 == 0;
  const bool v2 = xa % 8 == 0 && oa % 8 == 0 && ldx % 2 == 0 && ldo % 2 == 0;
  const int W = v4 ? 4 : 2;
  const int64_t G = ceil_div(F, W);
  const unsigned nb = (unsigned)ceil_div(rows * G, kTB);  // rows·G <= rows·P < 2^32: at most 2^24 blocks
  hipStream_t st = (hipStream_t)stream;
#define GNN_NOISE_LAUNCH(VEC)                                                                                     \
  noise_kernel<VEC><<<nb, kTB, 0, st>>>(x, ldx, (uint32_t)rows, (uint32_t)F, (uint32_t)G, (uint32_t)P, noise_std, \
                                        key_radius, key_angle, out, ldo)
  if (v4) GNN_NOISE_LAUNCH(4);
  else if (v2) GNN_NOISE_LAUNCH(2);
  else GNN_NOISE_LAUNCH(1);
#undef GNN_NOISE_LAUNCH
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}
