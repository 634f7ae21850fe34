// K20 — the feature-only baseline on the device (additive to ABI 32): what src/train_baselines.py and
// src/utils/calibrate.py:32-47 of the reference compute with sklearn, as the definitions of logreg.py /
// calibrate.py (the host mirrors there are these kernels' oracle).
//
// gnn_column_moments: mu and sd (population, two passes) of the columns of x over a row list, f64.  One
//     thread per column walks the block's GNN_LOGREG_ROWS rows; the blocks' partial sums are added in
//     block order by one thread per column.
// gnn_logreg_eval: F, g, H of the L2-penalised logistic objective at theta over the standardised rows
//     (z formed on the fly, never stored).  Each block takes GNN_LOGREG_ROWS rows in chunks of kChunk:
//     the chunk's z (with the constant 1 column) is staged in LDS as f64, one wave per row forms
//     t = z.w + b, one lane per row the row's terms, and then every thread adds its 8 x 8 register
//     tile of the LOWER triangle of sum h_i a_i a_i^T with f64 FMAs.  A block writes its (F, g, tiles)
//     slab; a second launch adds the slabs in slab order, scales by C, adds the penalty and mirrors the
//     triangle.  No float atomics, no hand-off between blocks inside a launch.  More than 256 tiles
//     (D + 1 > 176) are split over blockIdx.y: those blocks stage the same rows again (from L2).
// gnn_logreg_predict: sigma(z.w + b) per listed row, one wave per row.
// gnn_isotonic_fit: the tie groups of a one-segment rank plan read in ascending score order (a scan over
//     the plan's flags gives each group its first position and the positives before it, so a block of
//     groups [s, e) has W = first[e] - first[s] and P likewise: integers), PAVA on int64 cross products —
//     one thread per chunk of GNN_ISOTONIC_CHUNK groups, then one launch per level of pairwise merges in
//     which a thread per seam pools outward from its seam only — and the trim + compaction (a scan over
//     the keep flags).  A block's value is the one f64 division P / W: the same bits as the host mirror.
// gnn_isotonic_apply: scipy's linear interp1d as sklearn calls it, each f64 operation rounded once.
//
// Built with -ffp-contract=off: the interpolation and the standardisation are the mirror's operations;
// the accumulations that want an FMA call fma() themselves.
#include "common.hpp"
#include "rank_scan.hpp"

namespace gnnmp {
namespace {

constexpr int kTB = 256;
constexpr int kNW = kTB / kWave;
constexpr int kRows = GNN_LOGREG_ROWS;    // rows per block = per slab
constexpr int kChunk = 16;                // rows staged in LDS at a time
constexpr int kTile = 8;                  // a thread's H tile is kTile x kTile
constexpr int kMaxDp = 256;               // D + 1 rounded up to kTile, at most
constexpr int kHead = kMaxDp + 8;         // slab: [0] F, [8 .. 8 + Dp) g, [kHead + 64 q ..) tile q
constexpr int kUnroll = GNN_LOGREG_REDUCE_UNROLL;
static_assert(GNN_LOGREG_MAX_D + 1 <= kMaxDp && kMaxDp % kTile == 0 && kRows % kChunk == 0, "tile geometry");
static_assert(kChunk % kNW == 0, "a wave takes whole rows of a chunk");

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

inline int dp_of(int64_t D) { return (int)((D + 1 + kTile - 1) / kTile * kTile); }
inline int tiles_of(int64_t D) {
  const int T = dp_of(D) / kTile;
  return T * (T + 1) / 2;
}
inline size_t slab_doubles(int64_t D) { return (size_t)kHead + (size_t)tiles_of(D) * kTile * kTile; }

// the listed row k, or -1 (and the status bit) when it is outside x
__device__ __forceinline__ int64_t row_of(const int32_t* __restrict__ rows, int64_t k, int64_t num_rows,
                                          int32_t* __restrict__ status) {
  const int64_t r = rows ? (int64_t)rows[k] : k;
  if (r < 0 || r >= num_rows) {
    atomicOr(status, GNN_BASELINE_STATUS_ROW);
    return -1;
  }
  return r;
}

// the slabs' element at offset off, added in slab order (kUnroll loads in flight, one chain of adds)
__device__ __forceinline__ double slab_sum(const double* __restrict__ slabs, int64_t nb, int64_t stride, int64_t off) {
  double s = 0.0;
  int64_t b = 0;
  for (; b + kUnroll <= nb; b += kUnroll) {
    double v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) v[u] = slabs[(b + u) * stride + off];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) s = s + v[u];
  }
  for (; b < nb; ++b) s = s + slabs[b * stride + off];
  return s;
}

// ------------------------------------------------------------------------ column moments
// pass 0: part[b][j] = sum of x over the block's rows; pass 1: sum of (x - mu_j)^2
__global__ __launch_bounds__(kTB) void moments_part_kernel(const float* __restrict__ x, int64_t ld, int64_t num_rows,
                                                           const int32_t* __restrict__ rows, int64_t n, int64_t D,
                                                           const double* __restrict__ mu, int pass,
                                                           double* __restrict__ part, int32_t* __restrict__ status) {
  const int64_t j = threadIdx.x;
  if (j >= D) return;
  const int64_t k0 = blockIdx.x * (int64_t)kRows, k1 = k0 + kRows < n ? k0 + kRows : n;
  const double m = pass ? mu[j] : 0.0;
  double acc = 0.0;
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t r = row_of(rows, k, num_rows, status);
    if (r < 0) continue;
    const double v = (double)x[r * ld + j];
    if (pass) {
      const double d = v - m;
      acc = acc + d * d;
    } else {
      acc = acc + v;
    }
  }
  part[blockIdx.x * D + j] = acc;
}

__global__ __launch_bounds__(kTB) void moments_finish_kernel(const double* __restrict__ part, int64_t nb, int64_t n,
                                                             int64_t D, int pass, double* __restrict__ out) {
  const int64_t j = threadIdx.x;
  if (j >= D) return;
  const double v = slab_sum(part, nb, D, j) / (double)n;
  out[j] = pass ? (v == 0.0 ? 1.0 : __dsqrt_rn(v)) : v;
}

// ------------------------------------------------------------------------ logistic objective
struct RowTerms {
  double f, r, h, p;
};

// the row's terms from t = z.w + b through e = exp(-|t|): p = sigma(t), q = sigma(-t),
// f = s (softplus(t) - y t), r = s (p - y) (as -s q for y = 1), h = s p q
__device__ __forceinline__ RowTerms row_terms(double t, bool y, double s) {
  const double e = exp(-fabs(t)), d = 1.0 + e;
  const double p = t >= 0.0 ? 1.0 / d : e / d;
  const double q = t >= 0.0 ? e / d : 1.0 / d;
  const double sp = fmax(t, 0.0) + log1p(e);
  RowTerms o;
  o.f = s * (y ? sp - t : sp);
  o.r = y ? -(s * q) : s * p;
  o.h = s * (p * q);
  o.p = p;
  return o;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, kWave);
  return v;
}

template <bool FULL>
__global__ __launch_bounds__(kTB) void logreg_slab_kernel(const float* __restrict__ x, int64_t ld, int64_t num_rows,
                                                          const int32_t* __restrict__ rows, int64_t n, int D,
                                                          const uint8_t* __restrict__ y,
                                                          const double* __restrict__ mu,
                                                          const double* __restrict__ sd, double w0, double w1,
                                                          const double* __restrict__ theta,
                                                          double* __restrict__ slabs, int64_t slab_stride,
                                                          int32_t* __restrict__ status) {
  extern __shared__ double lds[];
  const int D1 = D + 1, Dp = (D1 + kTile - 1) / kTile * kTile;
  double* zs = lds;                  // [kChunk][Dp]
  double* th = zs + kChunk * Dp;     // [Dp]
  double* fr = th + Dp;              // [kChunk] each: f, r, h and t of the chunk's rows
  double* rr = fr + kChunk;
  double* hr = rr + kChunk;
  double* ts = hr + kChunk;
  double* ms = ts + kChunk;          // [Dp] each: mu and sd (0 and 1 for raw columns: (v - 0) / 1 is v)
  double* ss = ms + Dp;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  for (int j = tid; j < Dp; j += kTB) {
    th[j] = j < D1 ? theta[j] : 0.0;
    ms[j] = (mu && j < D) ? mu[j] : 0.0;
    ss[j] = (sd && j < D) ? sd[j] : 1.0;
  }

  // this thread's tile (ti >= tj) of the lower triangle
  const int T = Dp / kTile, q = blockIdx.y * kTB + tid;
  int ti = 0, tj = 0;
  bool has_tile = false;
  if (FULL && q < T * (T + 1) / 2) {
    has_tile = true;
    while ((ti + 1) * (ti + 2) / 2 <= q) ++ti;
    tj = q - ti * (ti + 1) / 2;
  }
  double acc[kTile][kTile];
#pragma unroll
  for (int u = 0; u < kTile; ++u)
#pragma unroll
    for (int v = 0; v < kTile; ++v) acc[u][v] = 0.0;
  double gacc = 0.0, facc = 0.0;

  const int64_t k0 = blockIdx.x * (int64_t)kRows, k1 = k0 + kRows < n ? k0 + kRows : n;
  for (int64_t c0 = k0; c0 < k1; c0 += kChunk) {
    __syncthreads();  // the last chunk's readers are done (and th, ms, ss are written)
    // a wave per row: the row's z from global memory (loads of one row independent of each other), kept
    // in LDS for the g and H passes, and t = z.w + b from the same registers
#pragma unroll
    for (int i = wid; i < kChunk; i += kNW) {
      const int64_t k = c0 + i;
      int64_t rix = -1;
      if (k < k1) {
        rix = rows ? (int64_t)rows[k] : k;
        if (rix < 0 || rix >= num_rows) rix = -1;
      }
      double part = 0.0;
#pragma unroll 4
      for (int j = lane; j < Dp; j += kWave) {
        double v = 0.0;
        if (rix >= 0) {
          if (j < D) v = ((double)x[rix * ld + j] - ms[j]) / ss[j];
          else if (j == D) v = 1.0;
        }
        if (FULL) zs[i * Dp + j] = v;
        part = fma(v, th[j], part);  // (th is 0 on the padding)
      }
      const double t = wave_sum(part);
      if (lane == 0) ts[i] = t;
    }
    __syncthreads();
    if (tid < kChunk) {  // the chunk's rows side by side: one lane each for exp and log1p
      const int64_t k = c0 + tid;
      RowTerms o = {0.0, 0.0, 0.0, 0.0};
      if (k < k1) {
        const int64_t rix = row_of(rows, k, num_rows, status);
        if (rix >= 0) {
          const bool pos = y[rix] != 0;
          o = row_terms(ts[tid], pos, pos ? w1 : w0);
        }
      }
      fr[tid] = o.f;
      rr[tid] = o.r;
      hr[tid] = o.h;
    }
    __syncthreads();
    if (tid == 0 && blockIdx.y == 0)
      for (int i = 0; i < kChunk; ++i) facc = facc + fr[i];
    if (FULL) {
      if (blockIdx.y == 0 && tid < Dp)
        for (int i = 0; i < kChunk; ++i) gacc = fma(rr[i], zs[i * Dp + tid], gacc);
      if (has_tile) {
        for (int i = 0; i < kChunk; ++i) {
          const double h = hr[i];
          double a[kTile], b[kTile];
#pragma unroll
          for (int u = 0; u < kTile; ++u) {
            a[u] = h * zs[i * Dp + ti * kTile + u];
            b[u] = zs[i * Dp + tj * kTile + u];
          }
#pragma unroll
          for (int u = 0; u < kTile; ++u)
#pragma unroll
            for (int v = 0; v < kTile; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
        }
      }
    }
  }
  double* slab = slabs + blockIdx.x * slab_stride;
  if (blockIdx.y == 0) {
    if (tid == 0) slab[0] = facc;
    if (FULL && tid < Dp) slab[8 + tid] = gacc;
  }
  if (has_tile) {
    double* o = slab + kHead + (int64_t)q * (kTile * kTile);
#pragma unroll
    for (int u = 0; u < kTile; ++u)
#pragma unroll
      for (int v = 0; v < kTile; ++v) o[u * kTile + v] = acc[u][v];
  }
}

// element 0: F; 1 .. D1: g; then H row-major [D1][D1] (both halves read the lower triangle's sums)
__global__ __launch_bounds__(kTB) void logreg_reduce_kernel(const double* __restrict__ slabs, int64_t nb,
                                                            int64_t stride, int D, double C,
                                                            const double* __restrict__ theta, int value_only,
                                                            double* __restrict__ F, double* __restrict__ g,
                                                            double* __restrict__ H) {
  const int64_t e = blockIdx.x * (int64_t)kTB + threadIdx.x;
  const int64_t D1 = D + 1;
  if (e == 0) {
    double ww = 0.0;
    for (int j = 0; j < D; ++j) ww = fma(theta[j], theta[j], ww);
    *F = C * slab_sum(slabs, nb, stride, 0) + 0.5 * ww;
    return;
  }
  if (value_only) return;
  if (e <= D1) {
    const int64_t j = e - 1;
    g[j] = C * slab_sum(slabs, nb, stride, 8 + j) + (j < D ? theta[j] : 0.0);
    return;
  }
  const int64_t h = e - 1 - D1;
  if (h >= D1 * D1) return;
  const int64_t r = h / D1, c = h - r * D1;
  const int64_t hi = r > c ? r : c, lo = r > c ? c : r;
  const int64_t ti = hi / kTile, tj = lo / kTile, q = ti * (ti + 1) / 2 + tj;
  const int64_t off = kHead + q * (kTile * kTile) + (hi % kTile) * kTile + (lo % kTile);
  H[h] = C * slab_sum(slabs, nb, stride, off) + ((r == c && r < D) ? 1.0 : 0.0);
}

__global__ __launch_bounds__(kTB) void logreg_predict_kernel(const float* __restrict__ x, int64_t ld, int64_t num_rows,
                                                             const int32_t* __restrict__ rows, int64_t n, int D,
                                                             const double* __restrict__ mu,
                                                             const double* __restrict__ sd,
                                                             const double* __restrict__ theta,
                                                             double* __restrict__ p64, float* __restrict__ p32,
                                                             int32_t* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int64_t k = blockIdx.x * (int64_t)kNW + wid;
  if (k >= n) return;  // (the whole wave)
  const int64_t rix = rows ? (int64_t)rows[k] : k;
  const bool ok = rix >= 0 && rix < num_rows;
  double part = 0.0;
  if (ok)
    for (int j = lane; j < D; j += kWave) {
      double v = (double)x[rix * ld + j];
      if (mu) v = (v - mu[j]) / sd[j];
      part = fma(v, theta[j], part);
    }
  const double t = wave_sum(part) + theta[D];
  if (lane != 0) return;
  double p = quiet_nan();
  if (ok) {
    const double e = exp(-fabs(t)), d = 1.0 + e;
    p = t >= 0.0 ? 1.0 / d : e / d;
  } else {
    atomicOr(status, GNN_BASELINE_STATUS_ROW);
  }
  if (p64) p64[k] = p;
  if (p32) p32[k] = (float)p;
}

// ------------------------------------------------------------------------ isotonic: groups
struct Pair {
  int32_t a, b;
};
struct AddPair {
  __device__ __forceinline__ Pair operator()(const Pair& x, const Pair& y) const { return Pair{x.a + y.a, x.b + y.b}; }
};
constexpr int kItems = 4;
constexpr int kScanTile = kTB * kItems;

// What a scan reads at position t.  Ascending position t is plan position m - 1 - t (the plan is
// descending), so a tie group's first ascending position is the plan's last of the group.
struct GroupLoad {
  const int32_t* order;
  const uint8_t* flags;
  const uint8_t* pos;
  __device__ __forceinline__ Pair operator()(int64_t t, int64_t m) const {
    const int64_t pp = m - 1 - t;
    return Pair{(flags[pp] & kGroupEnd) ? 1 : 0, pos[order[pp]] != 0 ? 1 : 0};
  }
};
// keep point k: the first, the last, a block's first or a block's last (its value differs from a neighbour's)
struct KeepLoad {
  const uint8_t* bstart;
  __device__ __forceinline__ Pair operator()(int64_t k, int64_t G) const {
    const bool keep = k == 0 || k == G - 1 || bstart[k] != 0 || bstart[k + 1] != 0;
    return Pair{keep ? 1 : 0, 0};
  }
};

// local[t] = inclusive scan inside the tile, agg[b] = the tile's total; *count elements
template <typename Load>
__global__ __launch_bounds__(kTB) void scan_tile_kernel(Load load, const int32_t* __restrict__ count,
                                                        Pair* __restrict__ local, Pair* __restrict__ agg) {
  __shared__ Pair wt[kNW];
  const int64_t m = *count;
  const int64_t base = blockIdx.x * (int64_t)kScanTile + threadIdx.x * kItems;
  Pair e[kItems];
#pragma unroll
  for (int j = 0; j < kItems; ++j) e[j] = base + j < m ? load(base + j, m) : Pair{0, 0};
#pragma unroll
  for (int j = 1; j < kItems; ++j) e[j] = AddPair()(e[j - 1], e[j]);
  Pair ex, tot;
  block_scan<kNW>(e[kItems - 1], AddPair(), Pair{0, 0}, wt, &ex, &tot);
#pragma unroll
  for (int j = 0; j < kItems; ++j)
    if (base + j < m) local[base + j] = AddPair()(ex, e[j]);
  if (threadIdx.x == 0) agg[blockIdx.x] = tot;
}

// carry[b] = totals of the tiles before b; carry[nb] = everything
__global__ __launch_bounds__(kTB) void scan_carry_kernel(const Pair* __restrict__ agg, int64_t nb,
                                                         Pair* __restrict__ carry) {
  __shared__ Pair wt[kNW];
  Pair run{0, 0};
  for (int64_t b0 = 0; b0 < nb; b0 += kTB) {
    const int64_t b = b0 + threadIdx.x;
    Pair ex, tot;
    block_scan<kNW>(b < nb ? agg[b] : Pair{0, 0}, AddPair(), Pair{0, 0}, wt, &ex, &tot);
    if (b < nb) carry[b] = AddPair()(run, ex);
    run = AddPair()(run, tot);
  }
  if (threadIdx.x == 0) carry[nb] = run;
}

// group g: first[g] its first ascending position, ppre[g] the positives before it, gx[g] its score;
// first[G] = m, ppre[G] = P, *G
__global__ __launch_bounds__(kTB) void iso_group_kernel(const float* __restrict__ scores,
                                                        const int32_t* __restrict__ order,
                                                        const uint8_t* __restrict__ flags,
                                                        const uint8_t* __restrict__ pos,
                                                        const int32_t* __restrict__ seg_ptr, int64_t nb,
                                                        const Pair* __restrict__ local,
                                                        const Pair* __restrict__ carry, int32_t* __restrict__ first,
                                                        int32_t* __restrict__ ppre, double* __restrict__ gx,
                                                        int32_t* __restrict__ G, int64_t* __restrict__ K) {
  const int64_t t = blockIdx.x * (int64_t)kTB + threadIdx.x;
  const int64_t m = seg_ptr[1];
  if (t == 0) {
    const Pair tot = carry[nb];
    *G = m > 0 ? tot.a : 0;
    if (m > 0) {
      first[tot.a] = (int32_t)m;
      ppre[tot.a] = tot.b;
    } else {
      *K = 0;
    }
  }
  if (t >= m) return;
  const int64_t pp = m - 1 - t;
  if (!(flags[pp] & kGroupEnd)) return;
  const Pair c = carry[t / kScanTile], l = local[t];
  const int32_t e = order[pp];
  const int64_t g = (int64_t)c.a + l.a - 1;
  first[g] = (int32_t)t;
  ppre[g] = c.b + l.b - (pos[e] != 0 ? 1 : 0);
  gx[g] = (double)scores[e] + 0.0;  // -0.0 -> +0.0
}

// ------------------------------------------------------------------------ isotonic: PAVA
// blocks are group intervals [s, e): nxt[s] = e and prv[e] = s for the blocks of the current lists,
// bstart[g] != 0 exactly at their first groups.  mean[a0, a1) >= mean[a1, b1) by cross multiplication.
__device__ __forceinline__ bool pools(const int32_t* __restrict__ first, const int32_t* __restrict__ ppre, int64_t a0,
                                      int64_t a1, int64_t b1) {
  const int64_t Pa = ppre[a1] - ppre[a0], Wa = first[a1] - first[a0];
  const int64_t Pb = ppre[b1] - ppre[a1], Wb = first[b1] - first[a1];
  return Pa * Wb >= Pb * Wa;
}

__global__ __launch_bounds__(kWave) void iso_chunk_kernel(const int32_t* __restrict__ first,
                                                          const int32_t* __restrict__ ppre,
                                                          const int32_t* __restrict__ Gp, int32_t* __restrict__ nxt,
                                                          int32_t* __restrict__ prv, uint8_t* __restrict__ bstart) {
  const int64_t G = *Gp;
  const int64_t lo = (blockIdx.x * (int64_t)kWave + threadIdx.x) * GNN_ISOTONIC_CHUNK;
  if (lo >= G) return;
  const int64_t hi = lo + GNN_ISOTONIC_CHUNK < G ? lo + GNN_ISOTONIC_CHUNK : G;
  for (int64_t g = lo; g < hi; ++g) {
    int64_t s = g;
    const int64_t e = g + 1;
    while (s > lo) {
      const int64_t ps = prv[s];
      if (!pools(first, ppre, ps, s, e)) break;
      bstart[s] = 0;
      s = ps;
    }
    bstart[s] = 1;
    prv[e] = (int32_t)s;
    nxt[s] = (int32_t)e;
  }
}

// the seams half (2 j + 1): the lists of [seam - half, seam) and [seam, seam + half) become one
__global__ __launch_bounds__(kWave) void iso_merge_kernel(const int32_t* __restrict__ first,
                                                          const int32_t* __restrict__ ppre,
                                                          const int32_t* __restrict__ Gp, int64_t half,
                                                          int32_t* __restrict__ nxt, int32_t* __restrict__ prv,
                                                          uint8_t* __restrict__ bstart) {
  const int64_t G = *Gp;
  const int64_t j = blockIdx.x * (int64_t)kWave + threadIdx.x;
  const int64_t seam = half * (2 * j + 1);
  if (seam >= G) return;
  const int64_t lo = seam - half, hi = seam + half < G ? seam + half : G;
  int64_t s = prv[seam], e = nxt[seam];
  if (!pools(first, ppre, s, seam, e)) return;
  bstart[seam] = 0;
  bool changed = true;
  while (changed) {
    changed = false;
    if (s > lo) {
      const int64_t ps = prv[s];
      if (pools(first, ppre, ps, s, e)) {
        bstart[s] = 0;
        s = ps;
        changed = true;
      }
    }
    if (e < hi) {
      const int64_t ne = nxt[e];
      if (pools(first, ppre, s, e, ne)) {
        bstart[e] = 0;
        e = ne;
        changed = true;
      }
    }
  }
  nxt[s] = (int32_t)e;
  prv[e] = (int32_t)s;
}

__global__ __launch_bounds__(kTB) void iso_emit_kernel(const int32_t* __restrict__ first,
                                                       const int32_t* __restrict__ ppre,
                                                       const double* __restrict__ gx,
                                                       const int32_t* __restrict__ Gp,
                                                       const int32_t* __restrict__ nxt,
                                                       const int32_t* __restrict__ prv,
                                                       const uint8_t* __restrict__ bstart, int64_t nb,
                                                       const Pair* __restrict__ local,
                                                       const Pair* __restrict__ carry, double* __restrict__ xs,
                                                       double* __restrict__ ys, int64_t* __restrict__ K) {
  const int64_t k = blockIdx.x * (int64_t)kTB + threadIdx.x;
  const int64_t G = *Gp;
  if (k >= G) return;
  if (k == G - 1) *K = carry[nb].a;
  const bool start = bstart[k] != 0;
  if (!(k == 0 || k == G - 1 || start || bstart[k + 1] != 0)) return;
  const int64_t at = (int64_t)carry[k / kScanTile].a + local[k].a - 1;
  const int64_t s = start ? k : prv[k + 1], e = start ? nxt[k] : k + 1;
  xs[at] = gx[k];
  ys[at] = (double)(ppre[e] - ppre[s]) / (double)(first[e] - first[s]);
}

struct SizerAdapter {
  WorkspaceSizer s;
  template <typename T>
  T* take(size_t n) { s.take<T>(n); return nullptr; }
};

struct IsoLayout {
  Pair *local, *agg, *carry;
  int32_t *first, *ppre, *nxt, *prv, *G;
  double* gx;
  uint8_t* bstart;
};
template <typename C>
void carve_iso(C& c, int64_t n, IsoLayout* L) {
  const size_t n1 = (size_t)(n > 0 ? n : 1) + 1, nb = (size_t)ceil_div(n > 0 ? n : 1, kScanTile) + 1;
  auto a = c.template take<Pair>(n1);
  auto b = c.template take<Pair>(nb);
  auto d = c.template take<Pair>(nb);
  auto f = c.template take<int32_t>(n1);
  auto p = c.template take<int32_t>(n1);
  auto x = c.template take<int32_t>(n1);
  auto v = c.template take<int32_t>(n1);
  auto g = c.template take<int32_t>(1);
  auto gx = c.template take<double>(n1);
  auto bs = c.template take<uint8_t>(n1);
  if (L) { L->local = a; L->agg = b; L->carry = d; L->first = f; L->ppre = p; L->nxt = x; L->prv = v; L->G = g; L->gx = gx; L->bstart = bs; }
}

__global__ __launch_bounds__(kTB) void iso_apply_kernel(const double* __restrict__ xs, const double* __restrict__ ys,
                                                        const int64_t* __restrict__ Kp, const float* __restrict__ q,
                                                        int64_t n, double* __restrict__ o64, float* __restrict__ o32,
                                                        int32_t* __restrict__ status) {
  const int64_t i = blockIdx.x * (int64_t)kTB + threadIdx.x;
  if (i >= n) return;
  const int64_t K = *Kp;
  double x = (double)q[i], out;
  if (x != x) {
    atomicOr(status, GNN_BASELINE_STATUS_NAN);
    out = quiet_nan();
  } else if (K <= 0) {
    out = x;  // no fit: the identity
  } else if (K == 1) {
    out = ys[0];
  } else {
    const double x0 = xs[0], x1 = xs[K - 1];
    x = x < x0 ? x0 : (x > x1 ? x1 : x);
    int64_t lo = 0, hi = K;  // the first position with xs[pos] >= x
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (xs[mid] < x) lo = mid + 1;
      else hi = mid;
    }
    const int64_t j = lo < 1 ? 1 : (lo > K - 1 ? K - 1 : lo);
    const double xl = xs[j - 1], yl = ys[j - 1];
    const double slope = (ys[j] - yl) / (xs[j] - xl);
    out = slope * (x - xl) + yl;
  }
  if (o64) o64[i] = out;
  if (o32) o32[i] = (float)out;
}

gnn_status check_rows(const char* fn, const float* x, int64_t ld, int64_t num_rows, int64_t n, int64_t D) {
  if (n < 0 || D < 1 || num_rows < 0) return fail(GNN_ERR_INVALID_ARG, fn, "negative size or D < 1");
  if (D > GNN_LOGREG_MAX_D) return fail(GNN_ERR_INVALID_ARG, fn, "D above GNN_LOGREG_MAX_D");
  if (n >= INT32_MAX || num_rows >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, fn, "n exceeds int32 range");
  if (ld < D) return fail(GNN_ERR_INVALID_ARG, fn, "ld below D");
  if (n > 0 && !x) return fail(GNN_ERR_INVALID_ARG, fn, "null buffer");
  return GNN_OK;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" gnn_status gnn_column_moments_workspace_size(int64_t n, int64_t D, size_t* bytes) {
  if (!bytes || n < 0 || D < 1) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size, D < 1 or null output");
  if (D > GNN_LOGREG_MAX_D) return fail(GNN_ERR_INVALID_ARG, __func__, "D above GNN_LOGREG_MAX_D");
  *bytes = align_up((size_t)ceil_div(n > 0 ? n : 1, kRows) * (size_t)D * sizeof(double), 256) + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_column_moments(const float* x, int64_t ld, int64_t num_rows, const int32_t* rows,
                                         int64_t n, int64_t D, double* mu, double* sd, int32_t* status,
                                         void* workspace, size_t workspace_bytes, gnn_stream_t stream) {
  gnn_status s = check_rows(__func__, x, ld, num_rows, n, D);
  if (s != GNN_OK) return s;
  if (n == 0) return GNN_OK;
  if (!mu || !sd || !status) return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  const int64_t nb = ceil_div(n, kRows);
  WorkspaceCarver c(workspace, workspace_bytes);
  double* part = c.take<double>((size_t)nb * (size_t)D);
  if (!workspace || !c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  for (int pass = 0; pass < 2; ++pass) {
    moments_part_kernel<<<(unsigned)nb, kTB, 0, st>>>(x, ld, num_rows, rows, n, D, mu, pass, part, status);
    GNN_LAUNCH_CHECK();
    moments_finish_kernel<<<1, kTB, 0, st>>>(part, nb, n, D, pass, pass ? sd : mu);
    GNN_LAUNCH_CHECK();
  }
  return GNN_OK;
}

extern "C" gnn_status gnn_logreg_eval_workspace_size(int64_t n, int64_t D, size_t* bytes) {
  if (!bytes || n < 0 || D < 1) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size, D < 1 or null output");
  if (D > GNN_LOGREG_MAX_D) return fail(GNN_ERR_INVALID_ARG, __func__, "D above GNN_LOGREG_MAX_D");
  *bytes = align_up((size_t)ceil_div(n > 0 ? n : 1, kRows) * slab_doubles(D) * sizeof(double), 256) + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_logreg_eval(const float* x, int64_t ld, int64_t num_rows, const int32_t* rows, int64_t n,
                                      int64_t D, const uint8_t* y, const double* mu, const double* sd, double w0,
                                      double w1, double C, const double* theta, int32_t value_only, double* F,
                                      double* g, double* H, int32_t* status, void* workspace,
                                      size_t workspace_bytes, gnn_stream_t stream) {
  gnn_status s = check_rows(__func__, x, ld, num_rows, n, D);
  if (s != GNN_OK) return s;
  if (!(C > 0.0) || !(w0 >= 0.0) || !(w1 >= 0.0) || C - C != 0.0 || w0 - w0 != 0.0 || w1 - w1 != 0.0)
    return fail(GNN_ERR_INVALID_ARG, __func__, "C must be positive and the class weights non-negative, all finite");
  if ((mu == nullptr) != (sd == nullptr)) return fail(GNN_ERR_INVALID_ARG, __func__, "mu and sd go together");
  if (n == 0) return GNN_OK;
  if (!y || !theta || !F || !status || (!value_only && (!g || !H)))
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  const int64_t nb = ceil_div(n, kRows);
  const size_t stride = slab_doubles(D);
  WorkspaceCarver c(workspace, workspace_bytes);
  double* slabs = c.take<double>((size_t)nb * stride);
  if (!workspace || !c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int Dp = dp_of(D);
  const size_t lds = ((size_t)kChunk * Dp + 3 * Dp + 4 * kChunk) * sizeof(double);
  if (value_only) {
    logreg_slab_kernel<false><<<dim3((unsigned)nb, 1), kTB, lds, st>>>(x, ld, num_rows, rows, n, (int)D, y, mu, sd, w0, w1,
                                                                      theta, slabs, (int64_t)stride, status);
    GNN_LAUNCH_CHECK();
    logreg_reduce_kernel<<<1, kWave, 0, st>>>(slabs, nb, (int64_t)stride, (int)D, C, theta, 1, F, g, H);
  } else {
    const unsigned ny = (unsigned)ceil_div(tiles_of(D), kTB);
    logreg_slab_kernel<true><<<dim3((unsigned)nb, ny), kTB, lds, st>>>(x, ld, num_rows, rows, n, (int)D, y, mu, sd, w0, w1,
                                                                      theta, slabs, (int64_t)stride, status);
    GNN_LAUNCH_CHECK();
    const int64_t outs = 1 + (D + 1) + (D + 1) * (D + 1);
    logreg_reduce_kernel<<<(unsigned)ceil_div(outs, kTB), kTB, 0, st>>>(slabs, nb, (int64_t)stride, (int)D, C, theta, 0, F,
                                                                       g, H);
  }
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

extern "C" gnn_status gnn_logreg_predict(const float* x, int64_t ld, int64_t num_rows, const int32_t* rows,
                                         int64_t n, int64_t D, const double* mu, const double* sd,
                                         const double* theta, double* p64, float* p32, int32_t* status,
                                         gnn_stream_t stream) {
  gnn_status s = check_rows(__func__, x, ld, num_rows, n, D);
  if (s != GNN_OK) return s;
  if ((mu == nullptr) != (sd == nullptr)) return fail(GNN_ERR_INVALID_ARG, __func__, "mu and sd go together");
  if (n == 0) return GNN_OK;
  if (!theta || !status || (!p64 && !p32)) return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  logreg_predict_kernel<<<(unsigned)ceil_div(n, kNW), kTB, 0, (hipStream_t)stream>>>(x, ld, num_rows, rows, n, (int)D, mu,
                                                                                    sd, theta, p64, p32, status);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

extern "C" gnn_status gnn_isotonic_fit_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  if (n >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n exceeds int32 range");
  SizerAdapter a;
  carve_iso(a, n, nullptr);
  *bytes = a.s.used + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_isotonic_fit(const float* scores, const int32_t* order, const uint8_t* flags,
                                       const int32_t* seg_ptr, const uint8_t* positive, int64_t n,
                                       int64_t num_segments, double* xs, double* ys, int64_t* K, void* workspace,
                                       size_t workspace_bytes, gnn_stream_t stream) {
  if (n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n");
  if (n >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n exceeds int32 range");
  if (num_segments != 1) return fail(GNN_ERR_INVALID_ARG, __func__, "the plan must have one segment");
  if (n == 0) return GNN_OK;
  if (!scores || !order || !flags || !seg_ptr || !positive || !xs || !ys || !K)
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  WorkspaceCarver c(workspace, workspace_bytes);
  IsoLayout L;
  carve_iso(c, n, &L);
  if (!workspace || !c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = ceil_div(n, kScanTile);
  const unsigned ne = (unsigned)ceil_div(n, kTB);
  // groups: (starts, positives) scanned over the ascending positions
  scan_tile_kernel<<<(unsigned)nb, kTB, 0, st>>>(GroupLoad{order, flags, positive}, seg_ptr + 1, L.local, L.agg);
  GNN_LAUNCH_CHECK();
  scan_carry_kernel<<<1, kTB, 0, st>>>(L.agg, nb, L.carry);
  GNN_LAUNCH_CHECK();
  iso_group_kernel<<<ne, kTB, 0, st>>>(scores, order, flags, positive, seg_ptr, nb, L.local, L.carry, L.first, L.ppre,
                                      L.gx, L.G, K);
  GNN_LAUNCH_CHECK();
  // PAVA: chunks, then the levels of pairwise merges
  const int64_t chunks = ceil_div(n, GNN_ISOTONIC_CHUNK);
  iso_chunk_kernel<<<(unsigned)ceil_div(chunks, kWave), kWave, 0, st>>>(L.first, L.ppre, L.G, L.nxt, L.prv, L.bstart);
  GNN_LAUNCH_CHECK();
  for (int64_t half = GNN_ISOTONIC_CHUNK; half < n; half *= 2) {
    const int64_t seams = ceil_div(n, 2 * half);
    iso_merge_kernel<<<(unsigned)ceil_div(seams, kWave), kWave, 0, st>>>(L.first, L.ppre, L.G, half, L.nxt, L.prv,
                                                                        L.bstart);
    GNN_LAUNCH_CHECK();
  }
  // trim + compaction
  scan_tile_kernel<<<(unsigned)nb, kTB, 0, st>>>(KeepLoad{L.bstart}, L.G, L.local, L.agg);
  GNN_LAUNCH_CHECK();
  scan_carry_kernel<<<1, kTB, 0, st>>>(L.agg, nb, L.carry);
  GNN_LAUNCH_CHECK();
  iso_emit_kernel<<<ne, kTB, 0, st>>>(L.first, L.ppre, L.gx, L.G, L.nxt, L.prv, L.bstart, nb, L.local, L.carry, xs, ys, K);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

extern "C" gnn_status gnn_isotonic_apply(const double* xs, const double* ys, const int64_t* K, const float* queries,
                                         int64_t n, double* out64, float* out32, int32_t* status,
                                         gnn_stream_t stream) {
  if (n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n");
  if (n >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n exceeds int32 range");
  if (n == 0) return GNN_OK;
  if (!xs || !ys || !K || !queries || !status || (!out64 && !out32))
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  iso_apply_kernel<<<(unsigned)ceil_div(n, kTB), kTB, 0, (hipStream_t)stream>>>(xs, ys, K, queries, n, out64, out32, status);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}
