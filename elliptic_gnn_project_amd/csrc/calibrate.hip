// K17 — the evaluation record on the device: the temperature fit (TemperatureScaler.fit,
// src/utils/calibrate.py:8-30, as the minimiser of the validation NLL instead of LBFGS's stopping
// point), the PR / ROC curve metrics of one K14 rank plan (src/utils/metrics.py:14-46: ROC-AUC, the
// max-F1 and precision-target thresholds, recall at precision) and the threshold / calibration
// counts of one pass over the scores (metrics.py:17-19 F1 at a threshold, 48-66 ECE).
//
// Temperature: ONE workgroup of GNN_FIT_THREADS.  Its waves compact the included rows' margins
// m_i = z[i, y_i] - z[i, 1 - y_i] (f64) into the workspace in row order (ballot prefix inside a wave,
// wave counts combined in wave order), then every thread runs the same safeguarded Newton iteration
// on beta = 1 / T: per evaluation each thread sums its strided share of (f, g, h) in f64, a xor
// butterfly folds the wave, the wave sums meet in LDS and every thread adds them in wave order — one
// fixed tree, so all threads hold the same bits and take the same branch.  One block: nothing to
// wait for between blocks.
//
// Curve: gnn_rank_ap's walk (tiles of GNN_RANK_TILE: aggregate, carry, terms) with the tie group's
// negative count beside gtp; integer counts, f64 values formed from them by single divisions, and
// (value, position) argmax reductions that compare exactly — independent of the reduction order.
//
// Built with -ffp-contract=off: f1 = 2.0*prec*rec/(prec+rec+1e-12) and the ECE terms are the host
// mirror's rounded operations one by one.
#include "common.hpp"
#include "rank_scan.hpp"

namespace gnnmp {
namespace {

// ------------------------------------------------------------------------ temperature fit
constexpr int kFitTB = GNN_FIT_THREADS;
constexpr int kFitNW = kFitTB / kWave;
constexpr double kBetaLo = 0x1p-10, kBetaHi = 0x1p10, kFlatGrad = 1e-7, kStepTol = 0x1p-40;
constexpr int kFitMaxIt = 100;

struct FitEval {
  double f, g, h;
};

// (f, g, h)(beta) over the compacted margins m[0..n), n >= 1; every thread of the block calls it and
// every thread receives the same bits.  sigma and softplus through e = exp(-|t|), t = beta * m.
__device__ FitEval fit_eval(const double* __restrict__ m, int64_t n, double beta, double (*red)[3]) {
  double f = 0.0, g = 0.0, h = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += kFitTB) {
    const double mj = m[j], t = beta * mj;
    const double e = exp(-fabs(t)), d = 1.0 + e;
    const double sp = t >= 0.0 ? 1.0 / d : e / d;  // sigma(t)
    const double sn = t >= 0.0 ? e / d : 1.0 / d;  // sigma(-t)
    f += fmax(-t, 0.0) + log1p(e);
    g += mj * sn;
    h += (mj * mj) * (sp * sn);
  }
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) {
    f += __shfl_xor(f, s, kWave);
    g += __shfl_xor(g, s, kWave);
    h += __shfl_xor(h, s, kWave);
  }
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  __syncthreads();  // red may still be read from the previous evaluation
  if (lane == 0) {
    red[wid][0] = f;
    red[wid][1] = g;
    red[wid][2] = h;
  }
  __syncthreads();
  f = g = h = 0.0;
  for (int w = 0; w < kFitNW; ++w) {
    f += red[w][0];
    g += red[w][1];
    h += red[w][2];
  }
  const double dn = (double)n;
  return FitEval{f / dn, -(g / dn), h / dn};
}

__global__ __launch_bounds__(kFitTB) void temperature_fit_kernel(const float* __restrict__ logits, int64_t ld,
                                                                 const int64_t* __restrict__ y,
                                                                 const uint8_t* __restrict__ include, int64_t N,
                                                                 double* __restrict__ m, float* __restrict__ T,
                                                                 double* __restrict__ diag,
                                                                 int32_t* __restrict__ status) {
  __shared__ long long wcount[kFitNW];
  __shared__ double red[kFitNW][3];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  // wave w owns the rows [w * per, (w + 1) * per), per a multiple of the wave
  const int64_t per = (N + kFitNW * kWave - 1) / (kFitNW * kWave) * kWave;
  const int64_t r0 = wid * per < N ? wid * per : N;
  const int64_t r1 = r0 + per < N ? r0 + per : N;
  int32_t bits = 0;
  auto margin = [&](int64_t i, double* out) -> bool {
    if (i >= r1) return false;
    const int64_t yi = y[i];
    const bool lab = yi == 0 || yi == 1;
    if (include ? include[i] == 0 : !lab) return false;
    if (!lab) {
      bits |= GNN_FIT_STATUS_LABEL;
      return false;
    }
    const double v = (double)logits[i * ld + yi] - (double)logits[i * ld + 1 - yi];
    if (!(fabs(v) <= 1.79769313486231570815e308)) {  // a NaN or infinite logit
      bits |= GNN_FIT_STATUS_NAN;
      return false;
    }
    *out = v;
    return true;
  };
  long long cnt = 0;
  double v = 0.0;
  for (int64_t b = r0; b < r1; b += kWave) cnt += __popcll(__ballot(margin(b + lane, &v)));
  if (lane == 0) wcount[wid] = cnt;
  __syncthreads();
  int64_t pre = 0, n = 0;
  for (int w = 0; w < kFitNW; ++w) {
    if (w < wid) pre += wcount[w];
    n += wcount[w];
  }
  for (int64_t b = r0; b < r1; b += kWave) {
    const bool ok = margin(b + lane, &v);
    const unsigned long long mask = __ballot(ok);
    if (ok) m[pre + __popcll(mask & ((1ull << lane) - 1ull))] = v;
    pre += __popcll(mask);
  }
  if (bits) atomicOr(status, bits);
  __syncthreads();  // the margins are in place for every thread of the block

  double beta = 1.0;
  FitEval e{0.0, 0.0, 0.0};
  int it = 0;
  int32_t st = 0;
  if (n == 0) {
    st = GNN_FIT_STATUS_EMPTY;
  } else {
    e = fit_eval(m, n, 1.0, red);
    if (fabs(e.g) <= kFlatGrad) {
      st = GNN_FIT_STATUS_FLAT;
    } else {
      const FitEval lo_e = fit_eval(m, n, kBetaLo, red);
      if (lo_e.g >= 0.0) {
        st = GNN_FIT_STATUS_CLAMP_LOW;
        beta = kBetaLo;
        e = lo_e;
      } else {
        const FitEval hi_e = fit_eval(m, n, kBetaHi, red);
        if (hi_e.g <= 0.0) {
          st = GNN_FIT_STATUS_CLAMP_HIGH;
          beta = kBetaHi;
          e = hi_e;
        } else {
          double lo = kBetaLo, hi = kBetaHi;  // g(lo) < 0 < g(hi)
          for (;;) {
            if (e.g == 0.0) break;
            ++it;
            if (e.g < 0.0) lo = beta; else hi = beta;
            const double step = e.g / e.h;
            double cand = beta - step;
            // a Newton step below the tolerance ends the solve where it stands: beta is an end of the
            // bracket by now, and a candidate that rounds onto it must not fall back to the midpoint
            bool conv = e.h != 0.0 && fabs(step) <= kStepTol * beta;
            if (e.h == 0.0 || !(cand > lo && cand < hi)) cand = conv ? beta : 0.5 * (lo + hi);
            conv = conv || fabs(cand - beta) <= kStepTol * beta;
            beta = cand;
            e = fit_eval(m, n, beta, red);
            if (conv) break;
            if (it == kFitMaxIt) {
              st = GNN_FIT_STATUS_MAXIT;
              break;
            }
          }
        }
      }
    }
  }
  if (threadIdx.x == 0) {
    *T = (st & (GNN_FIT_STATUS_EMPTY | GNN_FIT_STATUS_FLAT)) ? 1.0f : (float)(1.0 / beta);
    diag[0] = beta;
    diag[1] = e.f;
    diag[2] = e.g;
    diag[3] = (double)it;
    if (st) atomicOr(status, st);
  }
}

// ------------------------------------------------------------------------ curve metrics
constexpr int kTB = 256;
constexpr int kItems = 4;
constexpr int kTile = GNN_RANK_TILE;
constexpr int kNW = kTB / kWave;
static_assert(kTB * kItems == kTile, "GNN_RANK_TILE is the scan blocks' tile");

struct Cur {  // tp / fp since the plan's start, gtp / gfp since the last group start
  int32_t grp, tp, fp, gtp, gfp;
};
struct CurOp {
  __device__ __forceinline__ Cur operator()(const Cur& a, const Cur& b) const {
    Cur r;
    r.grp = a.grp | b.grp;
    r.tp = a.tp + b.tp;
    r.fp = a.fp + b.fp;
    r.gtp = b.grp ? b.gtp : a.gtp + b.gtp;
    r.gfp = b.grp ? b.gfp : a.gfp + b.gfp;
    return r;
  }
};
static_assert(sizeof(Cur) == 20, "scan states move between lanes as 32-bit words");

struct CurvePart {  // one block's candidates
  double f1;        // largest f1 of its group ends (-1: none), at the largest such position
  long long f1_pos;
  long long hit_pos;  // largest group end with prec >= target (-1: none) and its TP
  long long hit_tp;
  long long auc;      // sum of gFP * (2 TP - gTP) over its group ends
};

struct CurTile {
  Cur e[kItems];
  uint8_t fl[kItems];
};

__device__ __forceinline__ void load_cur(const int32_t* __restrict__ order, const uint8_t* __restrict__ flags,
                                         const uint8_t* __restrict__ pos, int64_t m, int64_t base, CurTile& L) {
  const CurOp op;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int64_t t = base + j;
    if (t < m) {
      const uint8_t f = flags[t];
      const int32_t y = pos[order[t]] != 0;
      L.fl[j] = f;
      L.e[j] = Cur{(f & kGroupStart) ? 1 : 0, y, 1 - y, y, 1 - y};
    } else {
      L.fl[j] = 0;
      L.e[j] = Cur{0, 0, 0, 0, 0};
    }
  }
#pragma unroll
  for (int j = 1; j < kItems; ++j) L.e[j] = op(L.e[j - 1], L.e[j]);
}

__global__ __launch_bounds__(kTB) void curve_aggregate_kernel(const int32_t* __restrict__ order,
                                                              const uint8_t* __restrict__ flags,
                                                              const int32_t* __restrict__ seg_ptr,
                                                              const uint8_t* __restrict__ pos, Cur* __restrict__ agg) {
  __shared__ Cur wt[kNW];
  CurTile L;
  load_cur(order, flags, pos, seg_ptr[1], blockIdx.x * (int64_t)kTile + threadIdx.x * kItems, L);
  Cur ex, tot;
  block_scan<kNW>(L.e[kItems - 1], CurOp(), Cur{0, 0, 0, 0, 0}, wt, &ex, &tot);
  if (threadIdx.x == 0) agg[blockIdx.x] = tot;
}

// carry[b] = the state before block b; totals = {P, N} of the whole plan
__global__ __launch_bounds__(kTB) void curve_carry_kernel(const Cur* __restrict__ agg, int64_t nb,
                                                          Cur* __restrict__ carry, long long* __restrict__ totals) {
  __shared__ Cur wt[kNW];
  const CurOp op;
  const Cur ident{0, 0, 0, 0, 0};
  Cur run = ident;
  for (int64_t b0 = 0; b0 < nb; b0 += kTB) {
    const int64_t b = b0 + threadIdx.x;
    Cur ex, tot;
    block_scan<kNW>(b < nb ? agg[b] : ident, op, ident, wt, &ex, &tot);
    if (b < nb) carry[b] = op(run, ex);
    run = op(run, tot);
  }
  if (threadIdx.x == 0) {
    totals[0] = run.tp;
    totals[1] = run.fp;
  }
}

// the better of two (f1, position) candidates: larger f1, then larger position (the lower score)
__device__ __forceinline__ void take_f1(double& f1, long long& p, double of1, long long op_) {
  if (of1 > f1 || (of1 == f1 && op_ > p)) {
    f1 = of1;
    p = op_;
  }
}
__device__ __forceinline__ void take_hit(long long& p, long long& tp, long long op_, long long otp) {
  if (op_ > p) {
    p = op_;
    tp = otp;
  }
}

// CurvePart of the calling block's threads -> thread 0 (every thread calls it)
__device__ __forceinline__ CurvePart reduce_part(CurvePart v, CurvePart* wpart) {
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) {
    const double of1 = __shfl_xor(v.f1, s, kWave);
    const long long ofp = __shfl_xor(v.f1_pos, s, kWave);
    const long long ohp = __shfl_xor(v.hit_pos, s, kWave);
    const long long oht = __shfl_xor(v.hit_tp, s, kWave);
    v.auc += __shfl_xor(v.auc, s, kWave);
    take_f1(v.f1, v.f1_pos, of1, ofp);
    take_hit(v.hit_pos, v.hit_tp, ohp, oht);
  }
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) wpart[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kNW; ++w) {
      take_f1(v.f1, v.f1_pos, wpart[w].f1, wpart[w].f1_pos);
      take_hit(v.hit_pos, v.hit_tp, wpart[w].hit_pos, wpart[w].hit_tp);
      v.auc += wpart[w].auc;
    }
  return v;
}

__global__ __launch_bounds__(kTB) void curve_terms_kernel(const int32_t* __restrict__ order,
                                                          const uint8_t* __restrict__ flags,
                                                          const int32_t* __restrict__ seg_ptr,
                                                          const uint8_t* __restrict__ pos, double target,
                                                          const Cur* __restrict__ carry,
                                                          const long long* __restrict__ totals,
                                                          CurvePart* __restrict__ part) {
  __shared__ Cur wt[kNW];
  __shared__ CurvePart wpart[kNW];
  const CurOp op;
  const int64_t m = seg_ptr[1];
  const int64_t base = blockIdx.x * (int64_t)kTile + threadIdx.x * kItems;
  const long long P = totals[0];
  CurTile L;
  load_cur(order, flags, pos, m, base, L);
  Cur ex, tot;
  block_scan<kNW>(L.e[kItems - 1], op, Cur{0, 0, 0, 0, 0}, wt, &ex, &tot);
  ex = op(carry[blockIdx.x], ex);
  CurvePart v{-1.0, -1, -1, 0, 0};
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    if (base + j >= m || !(L.fl[j] & kGroupEnd)) continue;
    const Cur c = op(ex, L.e[j]);
    const double prec = (double)c.tp / (double)(c.tp + c.fp);  // tp + fp >= 1 at a valid position
    const double rec = P > 0 ? (double)c.tp / (double)P : 1.0;
    const double f1 = 2.0 * prec * rec / (prec + rec + 1e-12);
    take_f1(v.f1, v.f1_pos, f1, base + j);
    if (prec >= target) take_hit(v.hit_pos, v.hit_tp, base + j, c.tp);
    v.auc += (long long)c.gfp * (2ll * c.tp - c.gtp);
  }
  v = reduce_part(v, wpart);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

__global__ __launch_bounds__(kTB) void curve_finish_kernel(const int32_t* __restrict__ order,
                                                           const int32_t* __restrict__ seg_ptr,
                                                           const float* __restrict__ scores, double target,
                                                           const CurvePart* __restrict__ part, int64_t nb,
                                                           const long long* __restrict__ totals,
                                                           double* __restrict__ out) {
  __shared__ CurvePart wpart[kNW];
  CurvePart v{-1.0, -1, -1, 0, 0};
  for (int64_t b = threadIdx.x; b < nb; b += kTB) {
    const CurvePart o = part[b];
    take_f1(v.f1, v.f1_pos, o.f1, o.f1_pos);
    take_hit(v.hit_pos, v.hit_tp, o.hit_pos, o.hit_tp);
    v.auc += o.auc;
  }
  v = reduce_part(v, wpart);
  if (threadIdx.x != 0) return;
  const long long P = nb > 0 ? totals[0] : 0, N = nb > 0 ? totals[1] : 0;
  const double thr_f1 = v.f1_pos >= 0 ? (double)scores[order[v.f1_pos]] : 1.0;
  out[0] = thr_f1;
  out[1] = v.f1_pos >= 0 ? v.f1 : 0.0;
  out[2] = v.hit_pos >= 0 ? (double)scores[order[v.hit_pos]] : (1.0 >= target ? 1.0 : thr_f1);
  out[3] = v.hit_pos >= 0 ? (P > 0 ? (double)v.hit_tp / (double)P : 1.0) : 0.0;
  out[4] = (P > 0 && N > 0) ? (double)v.auc / (double)(2 * P * N) : __longlong_as_double(0x7ff8000000000000ll);
  out[5] = (double)P;
  out[6] = (double)N;
  out[7] = (double)seg_ptr[1];
}

struct CurveLayout {
  Cur *agg, *carry;
  CurvePart* part;
  long long* totals;
};
template <typename C>
void carve_curve(C& c, int64_t nb, CurveLayout* L) {
  auto a = c.template take<Cur>((size_t)nb);
  auto b = c.template take<Cur>((size_t)nb);
  auto p = c.template take<CurvePart>((size_t)nb);
  auto t = c.template take<long long>(2);
  if (L) {
    L->agg = a; L->carry = b; L->part = p; L->totals = t;
  }
}

struct SizerAdapter {
  WorkspaceSizer s;
  template <typename T>
  T* take(size_t n) { s.take<T>(n); return nullptr; }
};

// ------------------------------------------------------------------------ threshold / calibration counts
constexpr int kCalTB = 128;
constexpr int kCalItems = 32;
constexpr int kCalTile = kCalTB * kCalItems;  // elements per block
constexpr int kCalInts = 2 * GNN_CALIB_MAX_BINS + 3;  // LDS: count[b], positives[b], then TP, FP, FN

struct CalEdges {
  double e[GNN_CALIB_MAX_BINS + 1];
};

// Block b counts its kCalTile elements: the integers with LDS atomics, sum p per (bin, thread) in a
// column of its own (element order), the columns then folded per bin by one wave in a fixed tree.
__global__ __launch_bounds__(kCalTB) void calib_count_kernel(const float* __restrict__ scores,
                                                             const uint8_t* __restrict__ pos,
                                                             const uint8_t* __restrict__ include, int64_t n,
                                                             double thr, CalEdges E, int bins,
                                                             double* __restrict__ part,
                                                             long long* __restrict__ ipart) {
  extern __shared__ double sums[];  // [bins][kCalTB]
  __shared__ int cnt[kCalInts];
  const int tid = threadIdx.x;
  for (int i = tid; i < bins * kCalTB; i += kCalTB) sums[i] = 0.0;
  for (int i = tid; i < kCalInts; i += kCalTB) cnt[i] = 0;
  __syncthreads();
  const int64_t base = blockIdx.x * (int64_t)kCalTile;
  for (int j = 0; j < kCalItems; ++j) {
    const int64_t i = base + (int64_t)j * kCalTB + tid;
    if (i >= n || (include && include[i] == 0)) continue;
    const double p = (double)scores[i];
    const bool y = pos[i] != 0;
    int k = 0;
    for (int e = 0; e <= bins; ++e) k += E.e[e] <= p ? 1 : 0;  // searchsorted(edges, p, side="right")
    const int b = k - 1 < 0 ? 0 : (k - 1 > bins - 1 ? bins - 1 : k - 1);
    sums[b * kCalTB + tid] += p;
    atomicAdd(&cnt[b], 1);
    if (y) atomicAdd(&cnt[GNN_CALIB_MAX_BINS + b], 1);
    const bool pred = p >= thr;
    if (pred && y) atomicAdd(&cnt[2 * GNN_CALIB_MAX_BINS], 1);
    if (pred && !y) atomicAdd(&cnt[2 * GNN_CALIB_MAX_BINS + 1], 1);
    if (!pred && y) atomicAdd(&cnt[2 * GNN_CALIB_MAX_BINS + 2], 1);
  }
  __syncthreads();
  const int lane = tid & (kWave - 1), wid = tid / kWave;
  for (int b = wid; b < bins; b += kCalTB / kWave) {
    double v = sums[b * kCalTB + lane] + sums[b * kCalTB + kWave + lane];
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, kWave);
    if (lane == 0) part[blockIdx.x * (int64_t)bins + b] = v;
  }
  for (int i = tid; i < kCalInts; i += kCalTB) ipart[blockIdx.x * (int64_t)kCalInts + i] = cnt[i];
}
static_assert(kCalTB == 2 * kWave, "calib_count_kernel folds two columns per lane");

// Block partials in block order -> the outputs, f1 and ece.
__global__ __launch_bounds__(kCalInts <= 128 ? 128 : 256) void calib_finish_kernel(
    const double* __restrict__ part, const long long* __restrict__ ipart, int64_t nb, int bins,
    int64_t* __restrict__ counts, int64_t* __restrict__ bin_count, int64_t* __restrict__ bin_pos,
    double* __restrict__ bin_sum, double* __restrict__ out) {
  __shared__ long long ci[kCalInts];
  __shared__ double cs[GNN_CALIB_MAX_BINS];
  const int t = threadIdx.x;
  if (t < kCalInts) {
    long long s = 0;
    for (int64_t b = 0; b < nb; ++b) s += ipart[b * kCalInts + t];
    ci[t] = s;
  }
  if (t < bins) {
    double s = 0.0;
    for (int64_t b = 0; b < nb; ++b) s += part[b * bins + t];
    cs[t] = s;
  }
  __syncthreads();
  if (t < bins) {
    bin_count[t] = ci[t];
    bin_pos[t] = ci[GNN_CALIB_MAX_BINS + t];
    bin_sum[t] = cs[t];
  }
  if (t != 0) return;
  const long long tp = ci[2 * GNN_CALIB_MAX_BINS], fp = ci[2 * GNN_CALIB_MAX_BINS + 1],
                  fn = ci[2 * GNN_CALIB_MAX_BINS + 2];
  counts[0] = tp;
  counts[1] = fp;
  counts[2] = fn;
  long long n = 0;
  for (int b = 0; b < bins; ++b) n += ci[b];
  const long long den = 2 * tp + fp + fn;
  out[0] = den > 0 ? (double)(2 * tp) / (double)den : 0.0;
  double ece = 0.0;
  for (int b = 0; b < bins; ++b) {
    const long long c = ci[b];
    if (c == 0) continue;
    const double w = (double)c / (double)n;
    ece += w * fabs((double)ci[GNN_CALIB_MAX_BINS + b] / (double)c - cs[b] / (double)c);
  }
  out[1] = ece;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" gnn_status gnn_temperature_fit_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  *bytes = align_up((size_t)(n > 0 ? n : 1) * sizeof(double), 256);
  return GNN_OK;
}

extern "C" gnn_status gnn_temperature_fit(const float* logits, int64_t ld, const int64_t* y, const uint8_t* include,
                                          int64_t n, float* T, double* diag, int32_t* status, void* workspace,
                                          size_t workspace_bytes, gnn_stream_t stream) {
  if (n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n");
  if (ld < 2) return fail(GNN_ERR_INVALID_ARG, __func__, "row stride below the 2 classes");
  if (!T || !diag || !status || (n > 0 && (!logits || !y))) return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  if (!workspace || workspace_bytes < (size_t)(n > 0 ? n : 1) * sizeof(double))
    return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  temperature_fit_kernel<<<1, kFitTB, 0, (hipStream_t)stream>>>(logits, ld, y, include, n, (double*)workspace, T,
                                                                diag, status);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

extern "C" gnn_status gnn_rank_curve_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  SizerAdapter a;
  carve_curve(a, ceil_div(n > 0 ? n : 1, kTile), nullptr);
  *bytes = a.s.used + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_rank_curve(const int32_t* order, const uint8_t* flags, const int32_t* seg_ptr,
                                     const uint8_t* positive, const float* scores, int64_t n, int64_t num_segments,
                                     double target_precision, double* out, void* workspace, size_t workspace_bytes,
                                     gnn_stream_t stream) {
  if (n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n");
  if (n >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n exceeds int32 range");
  if (num_segments != 1) return fail(GNN_ERR_INVALID_ARG, __func__, "the plan must have one segment");
  if (target_precision != target_precision) return fail(GNN_ERR_INVALID_ARG, __func__, "target precision is NaN");
  if (!seg_ptr || !out || (n > 0 && (!order || !flags || !positive || !scores)))
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = n > 0 ? ceil_div(n, kTile) : 0;
  WorkspaceCarver c(workspace, workspace_bytes);
  CurveLayout L;
  carve_curve(c, nb > 0 ? nb : 1, &L);
  if (!c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  if (nb > 0) {
    curve_aggregate_kernel<<<nb, kTB, 0, st>>>(order, flags, seg_ptr, positive, L.agg);
    GNN_LAUNCH_CHECK();
    curve_carry_kernel<<<1, kTB, 0, st>>>(L.agg, nb, L.carry, L.totals);
    GNN_LAUNCH_CHECK();
    curve_terms_kernel<<<nb, kTB, 0, st>>>(order, flags, seg_ptr, positive, target_precision, L.carry, L.totals,
                                           L.part);
    GNN_LAUNCH_CHECK();
  }
  curve_finish_kernel<<<1, kTB, 0, st>>>(order, seg_ptr, scores, target_precision, L.part, nb, L.totals, out);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

extern "C" gnn_status gnn_threshold_calibration_workspace_size(int64_t n, int32_t bins, size_t* bytes) {
  if (!bytes || n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  if (bins < 1 || bins > GNN_CALIB_MAX_BINS) return fail(GNN_ERR_INVALID_ARG, __func__, "bins outside [1, GNN_CALIB_MAX_BINS]");
  const size_t nb = (size_t)ceil_div(n > 0 ? n : 1, kCalTile);
  *bytes = align_up(nb * bins * sizeof(double), 256) + align_up(nb * kCalInts * sizeof(long long), 256) + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_threshold_calibration(const float* scores, const uint8_t* positive, const uint8_t* include,
                                                int64_t n, double thr, const double* edges, int32_t bins,
                                                int64_t* counts, int64_t* bin_count, int64_t* bin_pos,
                                                double* bin_sum, double* out, void* workspace,
                                                size_t workspace_bytes, gnn_stream_t stream) {
  if (n < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n");
  if (bins < 1 || bins > GNN_CALIB_MAX_BINS) return fail(GNN_ERR_INVALID_ARG, __func__, "bins outside [1, GNN_CALIB_MAX_BINS]");
  if (!edges || !counts || !bin_count || !bin_pos || !bin_sum || !out || (n > 0 && (!scores || !positive)))
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  if (thr != thr || (double)(float)thr != thr) return fail(GNN_ERR_INVALID_ARG, __func__, "thr is not a float32 value");
  CalEdges E;
  for (int b = 0; b <= bins; ++b) {
    E.e[b] = edges[b];
    if (!(b == 0 || E.e[b] >= E.e[b - 1])) return fail(GNN_ERR_INVALID_ARG, __func__, "edges are not ascending");
  }
  for (int b = bins + 1; b <= GNN_CALIB_MAX_BINS; ++b) E.e[b] = 0.0;
  const int64_t nb = n > 0 ? ceil_div(n, kCalTile) : 0;
  WorkspaceCarver c(workspace, workspace_bytes);
  double* part = c.take<double>((size_t)(nb > 0 ? nb : 1) * bins);
  long long* ipart = c.take<long long>((size_t)(nb > 0 ? nb : 1) * kCalInts);
  if (!c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (nb > 0) {
    calib_count_kernel<<<nb, kCalTB, (size_t)bins * kCalTB * sizeof(double), st>>>(scores, positive, include, n, thr,
                                                                                  E, bins, part, ipart);
    GNN_LAUNCH_CHECK();
  }
  calib_finish_kernel<<<1, kCalInts <= 128 ? 128 : 256, 0, st>>>(part, ipart, nb, bins, counts, bin_count, bin_pos,
                                                                bin_sum, out);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}
