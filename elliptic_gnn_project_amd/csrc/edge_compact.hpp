// Stable compaction of the kept columns of edge_index[2, E] (contiguous int64), shared by the edge
// drop (perturb.hip, K15) and the hub ablation (hub.hip, K18): an exclusive scan of the keep flags
// gives every kept edge its output column, then both rows are copied.  The flags reach the scan through
// an input iterator (an int32 array for K15, edge_rank >= h evaluated on the fly for K18) and the
// copy through a predicate over the edge id; `kept` is the caller's count of kept edges.
#pragma once
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"

namespace gnnmp {

constexpr int kCompactTB = 256;

// keep(e) from an array of int32 flags
struct KeepFlag {
  const int32_t* keep;
  __device__ __forceinline__ bool operator()(int64_t e) const { return keep[e] != 0; }
};

template <class Keep>
__global__ __launch_bounds__(kCompactTB) void edge_compact_kernel(const int64_t* __restrict__ ei, int64_t E,
                                                                 int64_t kept, Keep keep,
                                                                 const int32_t* __restrict__ pos,
                                                                 int64_t* __restrict__ out) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= E || !keep(e)) return;
  const int64_t p = pos[e];  // the number of kept edges before e
  if (p >= kept) return;     // (a caller's count below the flags': nothing is written past out[2, kept])
  out[p] = ei[e];
  out[kept + p] = ei[E + e];
}

// temporary bytes of the scan below for E flags read through `flags` (only its type matters here)
template <class FlagIt>
gnn_status edge_compact_tmp_bytes(int64_t E, FlagIt flags, size_t* bytes) {
  const size_t n = (size_t)(E > 0 ? E : 1);
  size_t tb = 0;
  hipError_t err = rocprim::exclusive_scan(nullptr, tb, flags, (int32_t*)nullptr, 0, n, rocprim::plus<int32_t>(),
                                           (hipStream_t)0);
  if (err != hipSuccess) return hip_check(err, "edge_compact_tmp_bytes");
  *bytes = tb;
  return GNN_OK;
}

// pos[E] = exclusive scan of flags[0..E); out[2, kept] = the columns e of ei with keep(e), in order.
// E in [1, INT32_MAX); flags[e] must be 1 where keep(e) and 0 elsewhere.
template <class FlagIt, class Keep>
gnn_status edge_compact(const int64_t* ei, int64_t E, int64_t kept, FlagIt flags, Keep keep, int32_t* pos, void* tmp,
                        size_t tmp_bytes, int64_t* out, hipStream_t st) {
  size_t sb = tmp_bytes;
  GNN_HIP_TRY(rocprim::exclusive_scan(tmp, sb, flags, pos, 0, (size_t)E, rocprim::plus<int32_t>(), st));
  edge_compact_kernel<Keep><<<(unsigned)ceil_div(E, kCompactTB), kCompactTB, 0, st>>>(ei, E, kept, keep, pos, out);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

}  // namespace gnnmp
