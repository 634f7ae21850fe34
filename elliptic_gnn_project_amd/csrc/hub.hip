// K18 — hub ablation (src/analysis/hub_ablation.py:56-71, build_edge_index_ablated): the int(frac·N)
// nodes of highest in+out degree lose every incident edge.  Hub sets are nested, so ONE degree
// ranking answers every fraction:
//
//   deg[v]        = #{e : src[e] = v} + #{e : dst[e] = v}      (a self loop counts 2, duplicates each time)
//   order         = the nodes by (deg descending, node id ascending);  rank = its inverse
//   edge_rank[e]  = min(rank[src[e]], rank[dst[e]])
//   removed_cum[r] = #{e : edge_rank[e] <= r}
//
// and the graph without the h top hubs is the stable compaction of {e : edge_rank[e] >= h}, of
// E - removed_cum[h - 1] columns (the caller's `kept`): no host synchronisation in either call,
// nothing a stream capture cannot record.
//
// gnn_hub_rank:   init (deg = hist = 0, ids = 0..N-1) -> degree count (int32 atomic adds: integer sums,
//                 any order gives the same bits) -> one stable rocPRIM descending radix sort of
//                 (deg, node id) over the bits 2E can occupy; ids enter ascending, so stability is the
//                 tie rule -> inverse scatter -> per-edge min-rank with the histogram over edge_rank in
//                 the same pass (the top ranks' counters one cache line each) -> inclusive scan.
// gnn_hub_ablate: exclusive scan of (edge_rank >= h), evaluated by the scan's input iterator, and the
//                 compaction of both rows (edge_compact.hpp, shared with perturb.hip's edge drop).
//
// Node ids are trusted here (the Python wrapper checks 0 <= id < N once per ranking).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "common.hpp"
#include "edge_compact.hpp"

namespace gnnmp {
namespace {

constexpr int kTB = 256;

// The histogram over edge_rank keeps the first kPadRanks ranks kPadStride ints apart (one 128-byte line
// each) and the others densely behind them: the top hubs' counters receive most of the adds, and with 16
// of them in one line the pass measured 77 us against 35 us this way (full graph, DESIGN "Hub ablation").
constexpr int kPadRanks = 1024, kPadStride = 32;
__host__ __device__ __forceinline__ int64_t hist_slot(int32_t r) {
  return r < kPadRanks ? (int64_t)r * kPadStride : (int64_t)kPadRanks * (kPadStride - 1) + r;
}
inline size_t hist_slots(int64_t N) { return (size_t)(N > 0 ? N : 1) + (size_t)kPadRanks * (kPadStride - 1); }
struct HistAt {
  const int32_t* hist;
  __host__ __device__ __forceinline__ int32_t operator()(int32_t r) const { return hist[hist_slot(r)]; }
};
using HistIt = rocprim::transform_iterator<rocprim::counting_iterator<int32_t>, HistAt, int32_t>;

// one thread per histogram slot (slots >= N)
__global__ __launch_bounds__(kTB) void hub_init_kernel(int64_t N, int64_t slots, uint32_t* __restrict__ deg,
                                                       int32_t* __restrict__ hist, int32_t* __restrict__ ids) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v < slots) hist[v] = 0;
  if (v >= N) return;
  deg[v] = 0u;
  ids[v] = (int32_t)v;
}

__global__ __launch_bounds__(kTB) void hub_degree_kernel(const int64_t* __restrict__ ei, int64_t E,
                                                         uint32_t* __restrict__ deg) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= E) return;
  atomicAdd(&deg[ei[e]], 1u);
  atomicAdd(&deg[ei[E + e]], 1u);
}

// sorted position t holds node order[t]
__global__ __launch_bounds__(kTB) void hub_inverse_kernel(const int32_t* __restrict__ order, int64_t N,
                                                          int32_t* __restrict__ rank) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= N) return;
  rank[order[t]] = (int32_t)t;
}

__global__ __launch_bounds__(kTB) void hub_edge_rank_kernel(const int64_t* __restrict__ ei, int64_t E,
                                                            const int32_t* __restrict__ rank,
                                                            int32_t* __restrict__ edge_rank,
                                                            int32_t* __restrict__ hist) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int32_t a = rank[ei[e]], b = rank[ei[E + e]];
  const int32_t r = a < b ? a : b;  // in [0, N)
  edge_rank[e] = r;
  atomicAdd(&hist[hist_slot(r)], 1);
}

// the keep flag of edge e without the h top hubs, as the scan's input and the compaction's predicate
struct RankAtLeast {
  int32_t h;
  __host__ __device__ __forceinline__ int32_t operator()(int32_t r) const { return r >= h ? 1 : 0; }
};
struct KeepRank {
  const int32_t* edge_rank;
  int32_t h;
  __device__ __forceinline__ bool operator()(int64_t e) const { return edge_rank[e] >= h; }
};
using RankFlagIt = rocprim::transform_iterator<const int32_t*, RankAtLeast, int32_t>;

// the bits a degree can occupy: deg <= 2E
inline unsigned degree_bits(int64_t E) {
  unsigned b = 1;
  while (b < 32 && ((uint64_t)2 * (uint64_t)E >> b) != 0) ++b;
  return b;
}

struct RankLayout {
  uint32_t* deg_sorted;  // the sort's key output (unused afterwards)
  int32_t *ids, *hist;
  void* tmp;
  size_t tmp_bytes;
};

gnn_status rank_tmp_bytes(int64_t N, int64_t E, size_t* bytes) {
  const size_t n = (size_t)(N > 0 ? N : 1);
  size_t sb = 0, tb = 0;
  hipError_t err = rocprim::radix_sort_pairs_desc(nullptr, sb, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                                  (int32_t*)nullptr, (int32_t*)nullptr, n, 0, degree_bits(E),
                                                  (hipStream_t)0);
  if (err != hipSuccess) return hip_check(err, "rank_tmp_bytes (sort)");
  err = rocprim::inclusive_scan(nullptr, tb, HistIt(rocprim::counting_iterator<int32_t>(0), HistAt{nullptr}),
                                (int32_t*)nullptr, n, rocprim::plus<int32_t>(), (hipStream_t)0);
  if (err != hipSuccess) return hip_check(err, "rank_tmp_bytes (scan)");
  *bytes = sb > tb ? sb : tb;
  return GNN_OK;
}

struct SizerAdapter {
  WorkspaceSizer s;
  template <typename T>
  T* take(size_t n) { s.take<T>(n); return nullptr; }
};

template <typename C>
void carve_rank(C& c, int64_t N, size_t tmp_bytes, RankLayout* L) {
  const size_t n = (size_t)(N > 0 ? N : 1);
  auto k = c.template take<uint32_t>(n);
  auto i = c.template take<int32_t>(n);
  auto h = c.template take<int32_t>(hist_slots(N));
  auto t = c.template take<char>(tmp_bytes);
  if (L) { L->deg_sorted = k; L->ids = i; L->hist = h; L->tmp = (void*)t; L->tmp_bytes = tmp_bytes; }
}

template <typename C>
void carve_ablate(C& c, int64_t E, size_t tmp_bytes, int32_t** pos, void** tmp) {
  auto p = c.template take<int32_t>((size_t)(E > 0 ? E : 1));
  auto t = c.template take<char>(tmp_bytes);
  if (pos) *pos = p;
  if (tmp) *tmp = (void*)t;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" gnn_status gnn_hub_rank_workspace_size(int64_t num_nodes, int64_t num_edges, size_t* bytes) {
  if (!bytes || num_nodes < 0 || num_edges < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  if (num_nodes >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "num_nodes exceeds int32 range");
  if (num_edges >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "num_edges exceeds int32 range");
  size_t tb = 0;
  gnn_status s = rank_tmp_bytes(num_nodes, num_edges, &tb);
  if (s != GNN_OK) return s;
  SizerAdapter a;
  carve_rank(a, num_nodes, tb, nullptr);
  *bytes = a.s.used + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_hub_rank(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes, int32_t* deg,
                                   int32_t* order, int32_t* rank, int32_t* edge_rank, int32_t* removed_cum,
                                   void* workspace, size_t workspace_bytes, gnn_stream_t stream) {
  const int64_t E = num_edges, N = num_nodes;
  if (E < 0 || N < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative num_edges or num_nodes");
  if (E >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "num_edges exceeds int32 range");
  if (N >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "num_nodes exceeds int32 range");
  if (E == 0) return GNN_OK;  // no edge: nothing is launched or written (the caller knows this ranking)
  if (N == 0) return fail(GNN_ERR_INVALID_ARG, __func__, "edges without nodes");
  if (!edge_index || !deg || !order || !rank || !edge_rank || !removed_cum)
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  hipStream_t st = (hipStream_t)stream;
  {  // the arrays alone, before the device is asked for rocPRIM's temporary size
    WorkspaceCarver c0(workspace, workspace_bytes);
    carve_rank(c0, N, 0, (RankLayout*)nullptr);
    if (!workspace || !c0.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  }
  size_t tb = 0;
  gnn_status s = rank_tmp_bytes(N, E, &tb);
  if (s != GNN_OK) return s;
  WorkspaceCarver c(workspace, workspace_bytes);
  RankLayout L;
  carve_rank(c, N, tb, &L);
  if (!c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  const unsigned nbn = (unsigned)ceil_div(N, kTB), nbe = (unsigned)ceil_div(E, kTB);
  uint32_t* degu = reinterpret_cast<uint32_t*>(deg);  // deg <= 2E < 2^32: sorted as unsigned keys
  const int64_t slots = (int64_t)hist_slots(N);
  hub_init_kernel<<<(unsigned)ceil_div(slots, kTB), kTB, 0, st>>>(N, slots, degu, L.hist, L.ids);
  GNN_LAUNCH_CHECK();
  hub_degree_kernel<<<nbe, kTB, 0, st>>>(edge_index, E, degu);
  GNN_LAUNCH_CHECK();
  size_t sb = L.tmp_bytes;
  GNN_HIP_TRY(rocprim::radix_sort_pairs_desc(L.tmp, sb, degu, L.deg_sorted, L.ids, order, (size_t)N, 0, degree_bits(E),
                                             st));
  hub_inverse_kernel<<<nbn, kTB, 0, st>>>(order, N, rank);
  GNN_LAUNCH_CHECK();
  hub_edge_rank_kernel<<<nbe, kTB, 0, st>>>(edge_index, E, rank, edge_rank, L.hist);
  GNN_LAUNCH_CHECK();
  sb = L.tmp_bytes;
  GNN_HIP_TRY(rocprim::inclusive_scan(L.tmp, sb, HistIt(rocprim::counting_iterator<int32_t>(0), HistAt{L.hist}),
                                      removed_cum, (size_t)N, rocprim::plus<int32_t>(), st));
  return GNN_OK;
}

extern "C" gnn_status gnn_hub_ablate_workspace_size(int64_t num_edges, size_t* bytes) {
  if (!bytes || num_edges < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  if (num_edges >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "num_edges exceeds int32 range");
  size_t tb = 0;
  gnn_status s = edge_compact_tmp_bytes(num_edges, RankFlagIt(nullptr, RankAtLeast{0}), &tb);
  if (s != GNN_OK) return s;
  SizerAdapter a;
  carve_ablate(a, num_edges, tb, nullptr, nullptr);
  *bytes = a.s.used + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_hub_ablate(const int64_t* edge_index, int64_t num_edges, const int32_t* edge_rank,
                                     int64_t num_hubs, int64_t kept, int64_t* out, void* workspace,
                                     size_t workspace_bytes, gnn_stream_t stream) {
  const int64_t E = num_edges;
  if (E < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative num_edges");
  if (E >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "num_edges exceeds int32 range");
  // (the ranking's N is not an argument: a rank is an int32 below N < INT32_MAX, which bounds num_hubs)
  if (num_hubs < 0 || num_hubs >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "num_hubs outside [0, num_nodes]");
  if (kept < 0 || kept > E) return fail(GNN_ERR_INVALID_ARG, __func__, "kept outside [0, num_edges]");
  if (E == 0 || num_hubs == 0) return GNN_OK;  // nothing removed: the caller keeps edge_index itself
  if (kept == 0) return GNN_OK;                // nothing kept: nothing to write
  if (!edge_index || !edge_rank || !out) return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  hipStream_t st = (hipStream_t)stream;
  const RankAtLeast flag{(int32_t)num_hubs};
  {  // the positions alone, before the device is asked for rocPRIM's temporary size
    WorkspaceCarver c0(workspace, workspace_bytes);
    carve_ablate(c0, E, 0, nullptr, nullptr);
    if (!workspace || !c0.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  }
  size_t tb = 0;
  gnn_status s = edge_compact_tmp_bytes(E, RankFlagIt(edge_rank, flag), &tb);
  if (s != GNN_OK) return s;
  WorkspaceCarver c(workspace, workspace_bytes);
  int32_t* pos = nullptr;
  void* tmp = nullptr;
  carve_ablate(c, E, tb, &pos, &tmp);
  if (!c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  return edge_compact(edge_index, E, kept, RankFlagIt(edge_rank, flag), KeepRank{edge_rank, (int32_t)num_hubs}, pos, tmp,
                      tb, out, st);
}
