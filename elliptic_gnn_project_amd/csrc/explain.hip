// Explain-mode edge scores: the gradient of a per-edge message multiplier.
//
// PyG 2.5.3 MessagePassing.propagate, with `explain` on, multiplies every message by
// edge_mask[e] (sigmoid applied by the caller) before the aggregation; GNNExplainer then
// optimises the mask (src/analysis/explain.py:593-672 drives it).  For SAGEConv's mean,
// out_i = (sum_e m_e x_j) / max(deg_i, 1), so d m_e = <dOut_i, x_j> / max(deg_i, 1): a sampled
// dense-dense product over the CSR slots.  The forward and the x-gradient reuse the EDGE_W
// aggregation (K5/K6's alpha-weighted form) with the mask as the slot weight.
//
// One wavefront per CSR row: dOut_i stays in L1/L2 across its slots, each slot's x_j row is
// read once with coalesced loads (lane f, f+64, ...), the dot reduces by xor shuffles, and
// lane 0 writes the slot's score to its PyG edge id (csr_eid), so the output is in edge order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.hpp"

using namespace gnnmp;

namespace {

constexpr int kWavesPerBlock = 4;

__global__ void __launch_bounds__(64 * kWavesPerBlock)
edge_dot_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                const int32_t* __restrict__ eid, const float* __restrict__ nodew,
                const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb,
                int32_t F, int64_t N, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (r >= N) return;
  const float d = nodew ? fmaxf(nodew[r], 1.0f) : 1.0f;
  const float* ar = a + r * lda;
  const int32_t s1 = rowptr[r + 1];
  for (int32_t s = rowptr[r]; s < s1; ++s) {
    const float* bj = b + (int64_t)col[s] * ldb;
    float acc = 0.0f;
    for (int f = lane; f < F; f += 64) acc = fmaf(ar[f], bj[f], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) out[eid ? (int64_t)eid[s] : (int64_t)s] = acc / d;
  }
}

}  // namespace

extern "C" gnn_status gnn_edge_dot_f32(const gnn_graph* g, const int32_t* eid, const float* nodew,
                                       const float* a, int64_t lda, const float* b, int64_t ldb,
                                       int64_t F, float* out, gnn_stream_t stream) {
  if (!g || !out || (F > 0 && (!a || !b)) || F < 0 || F > INT32_MAX || lda < F || ldb < F)
    return fail(GNN_ERR_INVALID_ARG, __func__, "null pointer or bad width/leading dimension");
  const int64_t N = g->num_nodes;
  if (N == 0 || g->num_slots == 0) return GNN_OK;
  if (!g->rowptr || !g->col) return fail(GNN_ERR_INVALID_ARG, __func__, "graph without CSR");
  const int64_t blocks = (N + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(edge_dot_kernel, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0,
                     (hipStream_t)stream, g->rowptr, g->col, eid, nodew, a, lda, b, ldb, (int32_t)F, N,
                     out);
  return hip_check(hipGetLastError(), __func__);
}

// ---------------------------------------------------------------------------------------------
// K16 — the fused GNNExplainer mask step (gnnmp.h gnn_explain_step_params).  PyG 2.5.3
// GNNExplainer._train / _loss per epoch: sigmoid, the size and entropy regularisers over the hard
// entries, their backward and one torch.optim.Adam step — about 40 small torch launches over the
// [rows, F] node-feature mask and a host synchronisation for the boolean gather mask[hard].  Here
// one elementwise launch per mask: the regularisers' gradient is a closed form of the logit (the
// per-block means become per-block coefficients computed once from the hard counts), and the gate
// form folds the sigmoid gate's backward in front and the next epoch's h = x·sigmoid(mask) behind.
//
// One thread per group of VEC neighbouring columns of a row (the plain form is one row of n
// columns with a block id per column), K15's access rule: VEC 4 with 16-byte accesses, 2 with
// 8-byte ones, 1 by element; a row's last partial group goes element by element.  Per element it
// reads mask, exp_avg, exp_avg_sq (4 B each), grad or dh and x (4 / 8 B) and the hard byte, and
// writes mask, exp_avg, exp_avg_sq and h: 21 B in, 16 B out in the gate form.
namespace {

constexpr int kStepTB = 256;
constexpr float kExplainEps = 1e-15f;  // PyG GNNExplainer's EPS

struct StepArgs {
  int64_t rows, F, G;
  float* mask; int64_t ld_mask;
  const float* grad;  // plain form; gate form: dh
  int64_t ld_grad;
  const float* x; int64_t ld_x;
  float* h; int64_t ld_h;
  float *m1, *m2; int64_t ld_state;
  const uint8_t* hard; uint8_t* hard_out; int64_t ld_hard;
  const int32_t* block_of; int32_t B;
  const float *size_scale, *ent_scale;
  int32_t update;  // 0: only write h
  float step_size, bc2_sqrt, beta1, beta2, omb1, omb2, eps;  // omb = 1 - beta, formed in double
  int32_t* status;
};

template <int VEC> struct VecOf;
template <> struct VecOf<4> { using F = float4; using B = uint32_t; using I = int4; };
template <> struct VecOf<2> { using F = float2; using B = uint16_t; using I = int2; };
template <> struct VecOf<1> { using F = float; using B = uint8_t; using I = int32_t; };

template <int VEC, typename T>
__device__ __forceinline__ void load_group(const T* p, bool full, int cnt, T (&v)[VEC]) {
  using V = typename std::conditional<sizeof(T) == 1, typename VecOf<VEC>::B,
                                      typename std::conditional<std::is_same<T, float>::value, typename VecOf<VEC>::F,
                                                                typename VecOf<VEC>::I>::type>::type;
  if (VEC > 1 && full) {
    const V w = *reinterpret_cast<const V*>(p);
    __builtin_memcpy(v, &w, sizeof(V));
  } else {
#pragma unroll
    for (int q = 0; q < VEC; ++q) v[q] = q < cnt ? p[q] : T(0);
  }
}

template <int VEC, typename T>
__device__ __forceinline__ void store_group(T* p, bool vec, int cnt, const bool (&ok)[VEC], const T (&v)[VEC]) {
  using V = typename std::conditional<sizeof(T) == 1, typename VecOf<VEC>::B, typename VecOf<VEC>::F>::type;
  if (VEC > 1 && vec) {
    V w;
    __builtin_memcpy(&w, v, sizeof(V));
    *reinterpret_cast<V*>(p) = w;
  } else {
#pragma unroll
    for (int q = 0; q < VEC; ++q)
      if (q < cnt && ok[q]) p[q] = v[q];
  }
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.0f / (1.0f + expf(-v)); }

template <int VEC, bool GATE>
__global__ __launch_bounds__(kStepTB) void mask_step_kernel(const StepArgs a) {
  const int64_t t = blockIdx.x * (int64_t)kStepTB + threadIdx.x;
  if (t >= a.rows * a.G) return;
  const int64_t row = t / a.G, c0 = (t - row * a.G) * VEC;  // c0 < F: G = ceil(F / VEC)
  const int64_t left = a.F - c0;
  const int cnt = left < VEC ? (int)left : VEC;
  const bool full = cnt == VEC;

  int32_t blk[VEC];
  bool ok[VEC];
  bool all_ok = true;
  if constexpr (GATE) {
    const int32_t b = a.block_of[row];
#pragma unroll
    for (int q = 0; q < VEC; ++q) blk[q] = b;
  } else {
    load_group<VEC>(a.block_of + c0, full, cnt, blk);
  }
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    ok[q] = (uint32_t)blk[q] < (uint32_t)a.B;
    if (q < cnt && !ok[q]) all_ok = false;
    if (!ok[q]) blk[q] = 0;
  }
  if (!all_ok) *a.status = GNN_EXPLAIN_STATUS_BLOCK;  // (every writer stores the same word)
  if (GATE && !all_ok) return;                        // the whole row is skipped

  float mk[VEC], xv[VEC];
  load_group<VEC>(a.mask + row * a.ld_mask + c0, full, cnt, mk);
  if constexpr (GATE) load_group<VEC>(a.x + row * a.ld_x + c0, full, cnt, xv);
  if (a.update) {
    float gr[VEC], m1[VEC], m2[VEC];
    uint8_t hd[VEC];
    load_group<VEC>(a.grad + row * a.ld_grad + c0, full, cnt, gr);
    load_group<VEC>(a.m1 + row * a.ld_state + c0, full, cnt, m1);
    load_group<VEC>(a.m2 + row * a.ld_state + c0, full, cnt, m2);
    if (a.hard) load_group<VEC>(a.hard + row * a.ld_hard + c0, full, cnt, hd);
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      if (!ok[q]) continue;  // (stored element by element below: this one is left as it is)
      const float s = sigmoidf(mk[q]), sm = sigmoidf(-mk[q]);  // 1 - s without the cancellation
      float g = gr[q];
      if constexpr (GATE) g = g * xv[q] * (s * sm);
      if (!a.hard) {
        hd[q] = g != 0.0f ? 1 : 0;
      } else if (hd[q]) {
        const float se = s + kExplainEps, me = sm + kExplainEps;
        const float dent = -logf(se) - s / se + logf(me) + sm / me;
        g += (s * sm) * (a.size_scale[blk[q]] + a.ent_scale[blk[q]] * dent);
      }
      m1[q] = a.beta1 * m1[q] + a.omb1 * g;
      m2[q] = a.beta2 * m2[q] + a.omb2 * (g * g);
      mk[q] -= a.step_size * (m1[q] / (sqrtf(m2[q]) / a.bc2_sqrt + a.eps));
    }
    const bool vec = full && all_ok;
    store_group<VEC>(a.mask + row * a.ld_mask + c0, vec, cnt, ok, mk);
    store_group<VEC>(a.m1 + row * a.ld_state + c0, vec, cnt, ok, m1);
    store_group<VEC>(a.m2 + row * a.ld_state + c0, vec, cnt, ok, m2);
    if (!a.hard) store_group<VEC>(a.hard_out + row * a.ld_hard + c0, vec, cnt, ok, hd);
  }
  if constexpr (GATE) {
    if (a.h) {
      float hv[VEC];
#pragma unroll
      for (int q = 0; q < VEC; ++q) hv[q] = xv[q] * sigmoidf(mk[q]);
      store_group<VEC>(a.h + row * a.ld_h + c0, full, cnt, ok, hv);
    }
  }
}

inline bool aligned_to(const void* p, size_t a) { return p == nullptr || (uintptr_t)p % a == 0; }

}  // namespace

extern "C" gnn_status gnn_explain_mask_step_f32(const gnn_explain_step_params* p, gnn_stream_t stream) {
  if (!p) return fail(GNN_ERR_INVALID_ARG, __func__, "null params");
  const bool gate = p->x != nullptr;
  if (p->n < 0 || (gate && p->F < 0)) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n or F");
  if (p->t < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative step count t");
  if (p->num_blocks < 1) return fail(GNN_ERR_INVALID_ARG, __func__, "num_blocks below 1");
  if (p->t == 0 && (!gate || !p->h)) return fail(GNN_ERR_INVALID_ARG, __func__, "t = 0 only forms h (gate form with h)");
  if (!p->mask || !p->block_of || !p->status) return fail(GNN_ERR_INVALID_ARG, __func__, "null mask, block_of or status pointer");
  if (p->t > 0) {
    if (!(gate ? p->dh : p->grad) || !p->exp_avg || !p->exp_avg_sq)
      return fail(GNN_ERR_INVALID_ARG, __func__, "null gradient or moment pointer");
    if (!p->hard && !p->hard_out) return fail(GNN_ERR_INVALID_ARG, __func__, "epoch 0 (hard = NULL) needs hard_out");
    if (p->hard && (!p->size_scale || !p->ent_scale))
      return fail(GNN_ERR_INVALID_ARG, __func__, "hard without size_scale / ent_scale");
  }
  if (gate) {
    const int64_t F = p->F;
    if (p->ld_mask < F || p->ld_x < F || (p->h && p->ld_h < F) ||
        (p->t > 0 && (p->ld_dh < F || p->ld_state < F || p->ld_hard < F)))
      return fail(GNN_ERR_INVALID_ARG, __func__, "leading dimension below F");
  }
  StepArgs a{};
  a.rows = gate ? p->n : 1;
  a.F = gate ? p->F : p->n;
  if (a.rows == 0 || a.F == 0) return GNN_OK;
  a.mask = p->mask; a.x = p->x; a.h = gate ? p->h : nullptr;
  a.grad = gate ? p->dh : p->grad;
  a.m1 = p->exp_avg; a.m2 = p->exp_avg_sq;
  a.hard = p->hard; a.hard_out = p->hard_out;
  if (gate) {
    a.ld_mask = p->ld_mask; a.ld_grad = p->ld_dh; a.ld_x = p->ld_x; a.ld_h = p->ld_h;
    a.ld_state = p->ld_state; a.ld_hard = p->ld_hard;
  }
  a.block_of = p->block_of; a.B = p->num_blocks;
  a.size_scale = p->size_scale; a.ent_scale = p->ent_scale;
  a.update = p->t > 0;
  if (a.update) {
    const double bc1 = 1.0 - std::pow(p->beta1, (double)p->t);
    const double bc2 = 1.0 - std::pow(p->beta2, (double)p->t);
    a.step_size = (float)(p->lr / bc1);
    a.bc2_sqrt = (float)std::sqrt(bc2);
  } else {
    a.grad = nullptr; a.m1 = a.m2 = nullptr; a.hard = nullptr; a.hard_out = nullptr;
  }
  a.beta1 = (float)p->beta1; a.beta2 = (float)p->beta2; a.eps = (float)p->eps;
  a.omb1 = (float)(1.0 - p->beta1); a.omb2 = (float)(1.0 - p->beta2);
  a.status = p->status;
  // K15's rule over every array the call touches (the byte masks need VEC-byte alignment only)
  auto width_ok = [&](int v) {
    const size_t fb = 4 * (size_t)v;
    bool ok = aligned_to(a.mask, fb) && aligned_to(a.grad, fb) && aligned_to(a.x, fb) && aligned_to(a.h, fb) &&
              aligned_to(a.m1, fb) && aligned_to(a.m2, fb) && aligned_to(a.hard, v) && aligned_to(a.hard_out, v);
    if (!gate) return ok && aligned_to(a.block_of, fb);
    ok = ok && a.ld_mask % v == 0 && a.ld_x % v == 0 && (!a.h || a.ld_h % v == 0);
    if (a.update) ok = ok && a.ld_grad % v == 0 && a.ld_state % v == 0 && a.ld_hard % v == 0;
    return ok;
  };
  const int vec = width_ok(4) ? 4 : width_ok(2) ? 2 : 1;
  a.G = ceil_div(a.F, vec);
  if (a.G > INT64_MAX / a.rows || ceil_div(a.rows * a.G, kStepTB) > INT32_MAX)
    return fail(GNN_ERR_INVALID_ARG, __func__, "mask too large for one launch");
  const unsigned nb = (unsigned)ceil_div(a.rows * a.G, kStepTB);
  hipStream_t st = (hipStream_t)stream;
  with_vec(vec, [&](auto V) {
    if (gate) mask_step_kernel<decltype(V)::value, true><<<nb, kStepTB, 0, st>>>(a);
    else mask_step_kernel<decltype(V)::value, false><<<nb, kStepTB, 0, st>>>(a);
  });
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}
