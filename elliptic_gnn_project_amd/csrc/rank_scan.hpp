// The rank plan's position flags and the ordered block scan its walks share (rank_metrics.hip K14,
// calibrate.hip K17).
#pragma once
#include "common.hpp"

namespace gnnmp {

enum : uint8_t { kGroupEnd = 1, kSegStart = 2, kGroupStart = 4 };  // gnn_rank_plan_build's flags[t]

template <typename T>
__device__ __forceinline__ T shfl_up_words(const T& v, int d) {
  constexpr int W = sizeof(T) / 4;
  int w[W];
  T r;
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (int i = 0; i < W; ++i) w[i] = __shfl_up(w[i], d, kWave);
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}

// Exclusive prefix of v over the block's threads (thread order) and the block total, for any
// associative op: a shuffle scan inside each wave, then the wave totals combined serially in
// wave order — one fixed tree.  Every thread of the block calls it.
template <int NW, typename T, typename Op>
__device__ __forceinline__ void block_scan(const T& v, Op op, const T& ident, T* wave_tot, T* excl, T* total) {
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  T inc = v;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    T o = shfl_up_words(inc, d);
    if (lane >= d) inc = op(o, inc);
  }
  T ex = shfl_up_words(inc, 1);
  if (lane == 0) ex = ident;
  __syncthreads();  // wave_tot may still be read from an earlier scan
  if (lane == kWave - 1) wave_tot[wid] = inc;
  __syncthreads();
  T pre = ident, tot = ident;
  for (int w = 0; w < NW; ++w) {
    const T t = wave_tot[w];
    if (w < wid) pre = op(pre, t);
    tot = op(tot, t);
  }
  *excl = op(pre, ex);
  *total = tot;
}

}  // namespace gnnmp
