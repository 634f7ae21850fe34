// K19 — the run reports on the device (additive to ABI 32): the four pieces the tools of the reference's
// "Analysis" section need beyond K14 / K17 (src/analysis/workload_curves.py, eval_by_time.py,
// evaluate_ensemble.py; calibration_plots.py needs nothing new).
//
// gnn_rank_hits_at: the positives among the first k plan positions for a whole list of k: ONE inclusive
//     scan of the labels in plan order (per-tile block scans kept in the workspace, one block scanning
//     the tile totals into carries) and one gather per k.  Integer counts and one IEEE division.
// gnn_segment_threshold_counts: TP / FP / FN of (double)score >= thr and the element count per group:
//     a per-block LDS histogram (integer atomics) written to the block's row of the workspace, the rows
//     summed in block order by one thread per counter.  No sort, no plan, no global atomics.
// gnn_id_join: perm with other_ids[perm[i]] == base_ids[i]: two stable rocPRIM radix sorts of
//     (id, position) pairs, an element-wise comparison of the sorted keys and a scatter.  All 64 key bits
//     are sorted: the bits in use would take a host read of the largest id.
// gnn_ensemble_pair: the average of two runs' probabilities, or of their logits in the closed form
//     sigma((logit a + logit b) / 2) = r / (r + q), r = sqrt(a b), q = sqrt((1 - a)(1 - b)): multiply,
//     subtract, add, square root and divide, each correctly rounded in f64 — what numpy computes from the
//     same expression, bit for bit, which a log / exp chain could not promise.
//
// Built with -ffp-contract=off: every f64 operation is rounded on its own.
#include <rocprim/device/device_radix_sort.hpp>

#include "common.hpp"
#include "rank_scan.hpp"

namespace gnnmp {
namespace {

constexpr int kTB = 256;
constexpr int kItems = 4;
constexpr int kTile = GNN_RANK_TILE;
constexpr int kNW = kTB / kWave;
static_assert(kTB * kItems == kTile, "GNN_RANK_TILE is the scan blocks' tile");

struct AddI32 {
  __device__ __forceinline__ int32_t operator()(int32_t a, int32_t b) const { return a + b; }
};

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ------------------------------------------------------------------------ hits at a list of k
// local[t] = positives among the tile's positions up to t (inclusive), agg[b] = the tile's positives
__global__ __launch_bounds__(kTB) void hits_scan_kernel(const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ seg_ptr,
                                                        const uint8_t* __restrict__ pos, int32_t* __restrict__ local,
                                                        int32_t* __restrict__ agg) {
  __shared__ int32_t wt[kNW];
  const int64_t m = seg_ptr[1];
  const int64_t base = blockIdx.x * (int64_t)kTile + threadIdx.x * kItems;
  int32_t e[kItems];
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int64_t t = base + j;
    e[j] = (t < m && pos[order[t]] != 0) ? 1 : 0;
  }
#pragma unroll
  for (int j = 1; j < kItems; ++j) e[j] += e[j - 1];
  int32_t ex, tot;
  block_scan<kNW>(e[kItems - 1], AddI32(), 0, wt, &ex, &tot);
#pragma unroll
  for (int j = 0; j < kItems; ++j)
    if (base + j < m) local[base + j] = ex + e[j];
  if (threadIdx.x == 0) agg[blockIdx.x] = tot;
}

// carry[b] = positives before tile b
__global__ __launch_bounds__(kTB) void hits_carry_kernel(const int32_t* __restrict__ agg, int64_t nb,
                                                         int64_t* __restrict__ carry) {
  __shared__ int32_t wt[kNW];
  int64_t run = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += kTB) {
    const int64_t b = b0 + threadIdx.x;
    int32_t ex, tot;
    block_scan<kNW>(b < nb ? agg[b] : 0, AddI32(), 0, wt, &ex, &tot);
    if (b < nb) carry[b] = run + ex;
    run += tot;
  }
}

__global__ __launch_bounds__(kTB) void hits_gather_kernel(const int32_t* __restrict__ seg_ptr,
                                                          const int32_t* __restrict__ local,
                                                          const int64_t* __restrict__ carry,
                                                          const int64_t* __restrict__ ks, int64_t K,
                                                          int64_t* __restrict__ k_eff, int64_t* __restrict__ hits,
                                                          double* __restrict__ precision,
                                                          int32_t* __restrict__ status) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= K) return;
  const int64_t m = seg_ptr[1], k = ks[j];
  if (k < 1) {
    atomicOr(status, GNN_REPORT_STATUS_K);
    k_eff[j] = 0;
    hits[j] = 0;
    precision[j] = quiet_nan();
    return;
  }
  const int64_t ke = k < m ? k : m;
  int64_t h = 0;
  if (ke > 0) h = carry[(ke - 1) / kTile] + local[ke - 1];
  k_eff[j] = ke;
  hits[j] = h;
  precision[j] = ke > 0 ? (double)h / (double)ke : quiet_nan();
}

struct SizerAdapter {
  WorkspaceSizer s;
  template <typename T>
  T* take(size_t n) { s.take<T>(n); return nullptr; }
};

struct HitsLayout {
  int32_t *local, *agg;
  int64_t* carry;
};
template <typename C>
void carve_hits(C& c, int64_t n, HitsLayout* L) {
  const size_t n1 = (size_t)(n > 0 ? n : 1), nb = (size_t)ceil_div(n > 0 ? n : 1, kTile);
  auto a = c.template take<int32_t>(n1);
  auto b = c.template take<int32_t>(nb);
  auto d = c.template take<int64_t>(nb);
  if (L) { L->local = a; L->agg = b; L->carry = d; }
}

// ------------------------------------------------------------------------ threshold counts per group
constexpr int kSegTB = 256;
constexpr int kSegItems = 16;
constexpr int kSegTile = kSegTB * kSegItems;  // elements per block
static_assert((size_t)GNN_REPORT_MAX_SEGMENTS * 4 * sizeof(int32_t) <= 64 * 1024, "the LDS histogram of one block");

__global__ __launch_bounds__(kSegTB) void seg_count_kernel(const float* __restrict__ scores,
                                                           const uint8_t* __restrict__ pos,
                                                           const uint8_t* __restrict__ include,
                                                           const int32_t* __restrict__ segment, int64_t n, int64_t S,
                                                           double thr, int32_t* __restrict__ part,
                                                           int32_t* __restrict__ status) {
  extern __shared__ int32_t hist[];  // [S][4]: TP, FP, FN, elements
  const int64_t S4 = S * 4;
  for (int64_t i = threadIdx.x; i < S4; i += kSegTB) hist[i] = 0;
  __syncthreads();
  const int64_t base = blockIdx.x * (int64_t)kSegTile;
  int32_t bits = 0;
  for (int j = 0; j < kSegItems; ++j) {
    const int64_t i = base + (int64_t)j * kSegTB + threadIdx.x;
    if (i >= n || (include && include[i] == 0)) continue;
    const int64_t s = segment[i];
    if (s < 0 || s >= S) {
      bits |= GNN_RANK_STATUS_SEGMENT;
      continue;
    }
    const bool y = pos[i] != 0, pred = (double)scores[i] >= thr;
    if (pred && y) atomicAdd(&hist[s * 4 + 0], 1);
    if (pred && !y) atomicAdd(&hist[s * 4 + 1], 1);
    if (!pred && y) atomicAdd(&hist[s * 4 + 2], 1);
    atomicAdd(&hist[s * 4 + 3], 1);
  }
  if (bits) atomicOr(status, bits);
  __syncthreads();
  for (int64_t i = threadIdx.x; i < S4; i += kSegTB) part[blockIdx.x * S4 + i] = hist[i];
}

__global__ __launch_bounds__(kSegTB) void seg_finish_kernel(const int32_t* __restrict__ part, int64_t nb, int64_t S4,
                                                            int64_t* __restrict__ counts) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= S4) return;
  int64_t s = 0;
  for (int64_t b = 0; b < nb; ++b) s += part[b * S4 + i];
  counts[i] = s;
}

inline size_t seg_part_ints(int64_t n, int64_t S) {
  return (size_t)ceil_div(n > 0 ? n : 1, kSegTile) * (size_t)(S > 0 ? S : 1) * 4;
}

// ------------------------------------------------------------------------ join by id
__global__ __launch_bounds__(kTB) void join_init_kernel(const int64_t* __restrict__ base_ids,
                                                        const int64_t* __restrict__ other_ids, int64_t n,
                                                        int32_t* __restrict__ iota, int32_t* __restrict__ status) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  iota[i] = (int32_t)i;
  if (base_ids[i] < 0 || other_ids[i] < 0) atomicOr(status, GNN_JOIN_STATUS_NEGATIVE);
}

// sorted position t: base element pb[t] holds id kb[t], other element po[t] holds id ko[t]
__global__ __launch_bounds__(kTB) void join_match_kernel(const uint64_t* __restrict__ kb,
                                                         const uint64_t* __restrict__ ko,
                                                         const int32_t* __restrict__ pb,
                                                         const int32_t* __restrict__ po, int64_t n,
                                                         int32_t* __restrict__ perm, int32_t* __restrict__ status) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint64_t a = kb[t], b = ko[t];
  int32_t bits = 0;
  if (a != b) bits |= GNN_JOIN_STATUS_MISMATCH;
  if (t > 0 && (kb[t - 1] == a || ko[t - 1] == b)) bits |= GNN_JOIN_STATUS_DUPLICATE;
  if (bits) atomicOr(status, bits);
  perm[pb[t]] = po[t];  // pb is a permutation of 0..n-1 whatever the ids are
}

struct JoinLayout {
  uint64_t *kb, *ko;
  int32_t *iota, *pb, *po;
  void* tmp;
};
template <typename C>
void carve_join(C& c, int64_t n, size_t tmp_bytes, JoinLayout* L) {
  const size_t n1 = (size_t)(n > 0 ? n : 1);
  auto a = c.template take<uint64_t>(n1);
  auto b = c.template take<uint64_t>(n1);
  auto i = c.template take<int32_t>(n1);
  auto p = c.template take<int32_t>(n1);
  auto q = c.template take<int32_t>(n1);
  auto t = c.template take<char>(tmp_bytes);
  if (L) { L->kb = a; L->ko = b; L->iota = i; L->pb = p; L->po = q; L->tmp = (void*)t; }
}

gnn_status join_tmp_bytes(int64_t n, size_t* bytes) {
  size_t tb = 0;
  hipError_t err = rocprim::radix_sort_pairs(nullptr, tb, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                             (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)(n > 0 ? n : 1), 0, 64,
                                             (hipStream_t)0);
  if (err != hipSuccess) return hip_check(err, "join_tmp_bytes");
  *bytes = tb;
  return GNN_OK;
}

// ------------------------------------------------------------------------ pair ensemble
__global__ __launch_bounds__(kTB) void ensemble_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       const int32_t* __restrict__ perm_a, int64_t n, int mode,
                                                       float* __restrict__ out, int32_t* __restrict__ status) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t ia = i;
  if (perm_a) {
    ia = perm_a[i];
    if (ia < 0 || ia >= n) {
      atomicOr(status, GNN_RANK_STATUS_INDEX);
      out[i] = __uint_as_float(0x7fc00000u);
      return;
    }
  }
  float x = a[ia], y = b[i];
  if (x != x || y != y) {
    atomicOr(status, GNN_RANK_STATUS_NAN);
    out[i] = __uint_as_float(0x7fc00000u);
    return;
  }
  if (mode == GNN_ENSEMBLE_PROB) {
    out[i] = 0.5f * (x + y);
    return;
  }
  const float lo = (float)1e-6, hi = (float)(1.0 - 1e-6);  // numpy's clip bounds on f32 data
  x = x < lo ? lo : (x > hi ? hi : x);
  y = y < lo ? lo : (y > hi ? hi : y);
  const double da = (double)x, db = (double)y;
  const double r = __dsqrt_rn(da * db);
  const double q = __dsqrt_rn((1.0 - da) * (1.0 - db));
  out[i] = (float)__ddiv_rn(r, r + q);
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" gnn_status gnn_rank_hits_at_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  if (n >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n exceeds int32 range");
  SizerAdapter a;
  carve_hits(a, n, nullptr);
  *bytes = a.s.used + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_rank_hits_at(const int32_t* order, const int32_t* seg_ptr, const uint8_t* positive,
                                       int64_t n, int64_t num_segments, const int64_t* ks, int64_t num_k,
                                       int64_t* k_eff, int64_t* hits, double* precision, int32_t* status,
                                       void* workspace, size_t workspace_bytes, gnn_stream_t stream) {
  if (n < 0 || num_k < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n or num_k");
  if (n >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n exceeds int32 range");
  if (num_segments != 1) return fail(GNN_ERR_INVALID_ARG, __func__, "the plan must have one segment");
  if (num_k == 0) return GNN_OK;
  if (!seg_ptr || !ks || !k_eff || !hits || !precision || !status || (n > 0 && (!order || !positive)))
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  WorkspaceCarver c(workspace, workspace_bytes);
  HitsLayout L;
  carve_hits(c, n, &L);
  if (!workspace || !c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = n > 0 ? ceil_div(n, kTile) : 0;
  if (nb > 0) {
    hits_scan_kernel<<<(unsigned)nb, kTB, 0, st>>>(order, seg_ptr, positive, L.local, L.agg);
    GNN_LAUNCH_CHECK();
    hits_carry_kernel<<<1, kTB, 0, st>>>(L.agg, nb, L.carry);
    GNN_LAUNCH_CHECK();
  }
  hits_gather_kernel<<<(unsigned)ceil_div(num_k, kTB), kTB, 0, st>>>(seg_ptr, L.local, L.carry, ks, num_k, k_eff, hits,
                                                                    precision, status);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

extern "C" gnn_status gnn_segment_threshold_counts_workspace_size(int64_t n, int64_t num_segments, size_t* bytes) {
  if (!bytes || n < 0 || num_segments < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  if (num_segments > GNN_REPORT_MAX_SEGMENTS)
    return fail(GNN_ERR_INVALID_ARG, __func__, "num_segments above GNN_REPORT_MAX_SEGMENTS");
  *bytes = align_up(seg_part_ints(n, num_segments) * sizeof(int32_t), 256) + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_segment_threshold_counts(const float* scores, const uint8_t* positive,
                                                   const uint8_t* include, const int32_t* segment, int64_t n,
                                                   int64_t num_segments, double thr, int64_t* counts,
                                                   int32_t* status, void* workspace, size_t workspace_bytes,
                                                   gnn_stream_t stream) {
  const int64_t S = num_segments;
  if (n < 0 || S < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n or num_segments");
  if (S > GNN_REPORT_MAX_SEGMENTS) return fail(GNN_ERR_INVALID_ARG, __func__, "num_segments above GNN_REPORT_MAX_SEGMENTS");
  if (thr != thr || (double)(float)thr != thr) return fail(GNN_ERR_INVALID_ARG, __func__, "thr is not a float32 value");
  if (S == 0) return GNN_OK;  // no group: nothing to write
  if (!counts || !status || (n > 0 && (!scores || !positive || !segment)))
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  WorkspaceCarver c(workspace, workspace_bytes);
  int32_t* part = c.take<int32_t>(seg_part_ints(n, S));
  if (!workspace || !c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = n > 0 ? ceil_div(n, kSegTile) : 0;
  if (nb > 0) {
    seg_count_kernel<<<(unsigned)nb, kSegTB, (size_t)S * 4 * sizeof(int32_t), st>>>(scores, positive, include, segment,
                                                                                   n, S, thr, part, status);
    GNN_LAUNCH_CHECK();
  }
  seg_finish_kernel<<<(unsigned)ceil_div(S * 4, kSegTB), kSegTB, 0, st>>>(part, nb, S * 4, counts);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

extern "C" gnn_status gnn_id_join_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  if (n >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n exceeds int32 range");
  size_t tb = 0;
  gnn_status s = join_tmp_bytes(n, &tb);
  if (s != GNN_OK) return s;
  SizerAdapter a;
  carve_join(a, n, tb, nullptr);
  *bytes = a.s.used + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_id_join(const int64_t* base_ids, const int64_t* other_ids, int64_t n, int32_t* perm,
                                  int32_t* status, void* workspace, size_t workspace_bytes, gnn_stream_t stream) {
  if (n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n");
  if (n >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n exceeds int32 range");
  if (n == 0) return GNN_OK;
  if (!base_ids || !other_ids || !perm || !status) return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  {  // the arrays alone, before the device is asked for rocPRIM's temporary size
    WorkspaceCarver c0(workspace, workspace_bytes);
    carve_join(c0, n, 0, (JoinLayout*)nullptr);
    if (!workspace || !c0.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  }
  size_t tb = 0;
  gnn_status s = join_tmp_bytes(n, &tb);
  if (s != GNN_OK) return s;
  WorkspaceCarver c(workspace, workspace_bytes);
  JoinLayout L;
  carve_join(c, n, tb, &L);
  if (!c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)ceil_div(n, kTB);
  join_init_kernel<<<nb, kTB, 0, st>>>(base_ids, other_ids, n, L.iota, status);
  GNN_LAUNCH_CHECK();
  size_t sb = tb;
  GNN_HIP_TRY(rocprim::radix_sort_pairs(L.tmp, sb, reinterpret_cast<const uint64_t*>(base_ids), L.kb,
                                        (const int32_t*)L.iota, L.pb, (size_t)n, 0, 64, st));
  sb = tb;
  GNN_HIP_TRY(rocprim::radix_sort_pairs(L.tmp, sb, reinterpret_cast<const uint64_t*>(other_ids), L.ko,
                                        (const int32_t*)L.iota, L.po, (size_t)n, 0, 64, st));
  join_match_kernel<<<nb, kTB, 0, st>>>(L.kb, L.ko, L.pb, L.po, n, perm, status);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

extern "C" gnn_status gnn_ensemble_pair(const float* a, const float* b, const int32_t* perm_a, int64_t n,
                                        int32_t mode, float* out, int32_t* status, gnn_stream_t stream) {
  if (n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n");
  if (n >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n exceeds int32 range");
  if (mode != GNN_ENSEMBLE_PROB && mode != GNN_ENSEMBLE_LOGIT)
    return fail(GNN_ERR_INVALID_ARG, __func__, "mode is neither GNN_ENSEMBLE_PROB nor GNN_ENSEMBLE_LOGIT");
  if (n == 0) return GNN_OK;
  if (!a || !b || !out || !status) return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  ensemble_kernel<<<(unsigned)ceil_div(n, kTB), kTB, 0, (hipStream_t)stream>>>(a, b, perm_a, n, mode, out, status);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}
