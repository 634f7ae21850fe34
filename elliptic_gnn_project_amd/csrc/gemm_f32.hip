// K7 — fp32 MFMA GEMMs for the dense transforms of SAGEConv/GCNConv/GATConv, with the
// surrounding elementwise work of src/models/gnn.py fused in.
//
// Replaces PyG Linear (lin_l / lin_r / lin, gnn.py:41-44, 20-23, 64-67) and the ReLU +
// dropout between layers (gnn.py:29-30, 50-51) — forward (NT kernel) and weight
// gradients (TN kernel).  Exact fp32: v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain
// (no TF32/xf32 on gfx950), so results are within fp32 rounding of ATen's sgemm.
//
// NT:  C[M,Nc] = epi( [A1 | A2][M, k1+k2] · Bt[k1+k2, Nc] )
//      epi = +bias, ReLU, dropout (counter hash, keep prob 1-p, scale 1/(1-p)),
//      optional projection Z[M,nproj] = C · Pᵀ (P [nproj, Nc]) — the next, narrow layer's
//      transform-first GEMM computed from registers (the hidden activations' row is whole
//      in one wave).  gemm_nt2_kernel<AVEC, BVEC, WFORM>: block = 4 waves x (32 rows x 128 cols);
//      K streamed in 16-deep chunks (NT_KC) through double-buffered LDS, one chunk of loads in
//      flight, both operands K-contiguous rows read as b128 fragments.  AVEC / BVEC: widest row
//      vector of A / W (4, 2, 1); WFORM: B read in place from the Linear weights W1 / W2 [Nc, K],
//      else from a transposed copy Bt [K, Nc].
//      Measured and dropped (r01 lab, all slower): a [k][n] B image with scalar b32 fragment
//      reads (A padded to KC + 1 floats per row), 32-deep chunks, two chunks of loads in flight.
// TN:  dW[Nr, k1+k2] = Σ_m G[m, Nr]ᵀ · [A1 | A2][m, :]   (split over M, slabs, ordered reduce)
//      G = (G_src or dz·P) ⊙ (h > 0 ? scale : 0)   — ReLU+dropout backward computed on the fly
//      side sums: db[n] = Σ G, dW2[q][n] = Σ dz[m,q]·h[m,n], dzsum[q] = Σ dz[m,q]
//      Block = 16 waves: wave w owns dW rows (w&3)*32.. and k-tiles (w>>2)*3 .. +3.
// Both are atomic-free and deterministic.
#include "common.hpp"

#include <algorithm>

#include "gemm_common.hpp"

namespace gnnmp {
using gemm::aligned;
namespace {

// ------------------------------------------------------------ NT, k-permuted b128 fragments
// Both LDS images are K-contiguous rows — A as [row][k], B as [n][k] (the PyTorch Linear weight
// layout, so W is staged in place) — with a pitch of NT_KC + 4 floats.  MFMA k-step j of k-group g
// pairs k = 8g+j (lanes 0-31) with k = 8g+4+j (lanes 32-63): each lane fetches the operands of
// four k-steps with ONE ds_read_b128 (pitch ≡ 20 mod 64 dwords keeps the b128 lane groups
// conflict-free), 5 LDS reads per 16 MFMAs instead of 20.  Every k is still summed exactly once
// per output, in a fixed order, with zero-filled tails in both operands.
constexpr int NT_KC = 16;           // K depth of an LDS chunk
constexpr int NT_BM = 128;          // block rows (4 waves x 32)
constexpr int NT_P = NT_KC + 4;     // LDS row pitch, floats
constexpr int NT_AREG = NT_BM * NT_KC / 256, NT_BREG = BN * NT_KC / 256;  // staged floats per thread

// chunk c of [A1 | A2]: its operand, k origin in the segment (k0) and in Bt (kb0), and depth
__device__ __forceinline__ void nt_chunk_range(const NTArgs& a, int c, const float*& A, int64_t& lda, int& k0,
                                               int& kb0, int& klen) {
  constexpr int KC = NT_KC;
  const int nch1 = (a.k1 + KC - 1) / KC;
  if (c < nch1) { A = a.a1; lda = a.lda1; k0 = c * KC; kb0 = k0; klen = min(KC, a.k1 - k0); }
  else { A = a.a2; lda = a.lda2; k0 = (c - nch1) * KC; kb0 = a.k1 + k0; klen = min(KC, a.k2 - k0); }
}

// Stage rows [r0, r0+128) x [k0, k0+KC) of a K-contiguous row-major operand into registers.
// Row and k are clamped (loads never depend on data: the prefetch stays in flight).
template <int VEC>
__device__ __forceinline__ void nt2_load_rows(const float* X, int64_t ldx, int64_t r0, int64_t rows, int k0,
                                              int klen, float* reg) {
  constexpr int KC = NT_KC, VPR = KC / VEC;
#pragma unroll
  for (int i = 0; i < 128 * KC / 256 / VEC; ++i) {
    const int v = threadIdx.x + 256 * i;
    const int r = v / VPR;
    const int k = (v % VPR) * VEC;
    int64_t row = r0 + r;
    row = row < rows ? row : rows - 1;
    const float* p = X + row * ldx + k0 + (k < klen ? k : 0);
    if constexpr (VEC == 4) {
      const float4 t = *reinterpret_cast<const float4*>(p);
      reg[i * 4 + 0] = t.x; reg[i * 4 + 1] = t.y; reg[i * 4 + 2] = t.z; reg[i * 4 + 3] = t.w;
    } else if constexpr (VEC == 2) {
      const float2 t = *reinterpret_cast<const float2*>(p);
      reg[i * 2 + 0] = t.x; reg[i * 2 + 1] = t.y;
    } else {
      reg[i] = *p;
    }
  }
}

template <int VEC>
__device__ __forceinline__ void nt2_store_rows(float* L, int64_t r0, int64_t rows, int klen, bool full,
                                               const float* reg) {
  constexpr int KC = NT_KC, VPR = KC / VEC, P = NT_P;
#pragma unroll
  for (int i = 0; i < 128 * KC / 256 / VEC; ++i) {
    const int v = threadIdx.x + 256 * i;
    const int r = v / VPR;
    const int k = (v % VPR) * VEC;
    const bool ok = full || ((r0 + r < rows) && (k < klen));  // VEC divides klen: all-or-nothing
    float* d = L + r * P + k;
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(d) = ok ? make_float4(reg[i * 4], reg[i * 4 + 1], reg[i * 4 + 2], reg[i * 4 + 3])
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
    } else if constexpr (VEC == 2) {
      *reinterpret_cast<float2*>(d) = ok ? make_float2(reg[i * 2], reg[i * 2 + 1]) : make_float2(0.f, 0.f);
    } else {
      *d = ok ? reg[i] : 0.0f;
    }
  }
}

// B from the transposed copy Bt [K, Nc] (N-contiguous): lanes run along k so the transposed
// scalar LDS stores spread over the banks; k and n are clamped.
__device__ __forceinline__ void nt2_load_bt(const NTArgs& a, int kb0, int klen, int n0, bool bvec4, float* reg) {
  constexpr int KC = NT_KC;
#pragma unroll
  for (int i = 0; i < BN * KC / 256 / 4; ++i) {
    const int v = threadIdx.x + 256 * i;
    const int kk = v % KC;
    const int n = (v / KC) * 4;
    const float* p = a.bt + (int64_t)(kb0 + (kk < klen ? kk : 0)) * a.ldb;
    if (bvec4) {
      const int nn = n0 + n < a.Nc ? n0 + n : 0;
      const float4 t = *reinterpret_cast<const float4*>(p + nn);
      reg[i * 4 + 0] = t.x; reg[i * 4 + 1] = t.y; reg[i * 4 + 2] = t.z; reg[i * 4 + 3] = t.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) reg[i * 4 + q] = p[n0 + n + q < a.Nc ? n0 + n + q : 0];
    }
  }
}

__device__ __forceinline__ void nt2_store_bt(const NTArgs& a, float* L, int klen, int n0, const float* reg) {
  constexpr int KC = NT_KC, P = NT_P;
#pragma unroll
  for (int i = 0; i < BN * KC / 256 / 4; ++i) {
    const int v = threadIdx.x + 256 * i;
    const int kk = v % KC;
    const int n = (v / KC) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) L[(n + q) * P + kk] = (kk < klen && n0 + n + q < a.Nc) ? reg[i * 4 + q] : 0.0f;
  }
}

// one chunk of both operands in registers, between its loads and its LDS stores
template <int AVEC, int BVEC, bool WFORM>
struct NT2Stage {
  float ra[NT_AREG];
  float rb[NT_BREG];
  __device__ __forceinline__ void load(const NTArgs& a, int c, int64_t m0, int n0, bool bvec4) {
    constexpr int KC = NT_KC;
    const float* A; int64_t lda; int k0, kb0, klen;
    nt_chunk_range(a, c, A, lda, k0, kb0, klen);
    nt2_load_rows<AVEC>(A, lda, m0, a.M, k0, klen, ra);
    if constexpr (WFORM) {
      const bool seg1 = c < (a.k1 + KC - 1) / KC;
      nt2_load_rows<BVEC>(seg1 ? a.w1 : a.w2, seg1 ? a.ldw1 : a.ldw2, n0, a.Nc, k0, klen, rb);
    } else {
      nt2_load_bt(a, kb0, klen, n0, bvec4, rb);
    }
  }
  __device__ __forceinline__ void store(const NTArgs& a, int c, int64_t m0, int n0, float* As, float* Bs) {
    const float* A; int64_t lda; int k0, kb0, klen;
    nt_chunk_range(a, c, A, lda, k0, kb0, klen);
    const bool kfull = klen == NT_KC;
    nt2_store_rows<AVEC>(As, m0, a.M, klen, kfull && m0 + NT_BM <= a.M, ra);
    if constexpr (WFORM) nt2_store_rows<BVEC>(Bs, n0, a.Nc, klen, kfull && n0 + BN <= a.Nc, rb);
    else nt2_store_bt(a, Bs, klen, n0, rb);
  }
};

template <int AVEC, int BVEC, bool WFORM>
__global__ __launch_bounds__(256) void gemm_nt2_kernel(NTArgs a) {
  constexpr int KC = NT_KC, P = NT_P;
  __shared__ __attribute__((aligned(16))) float As[2][NT_BM * P];
  __shared__ __attribute__((aligned(16))) float Bs[2][BN * P];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * NT_BM;
  const int n0 = blockIdx.y * BN;
  const int nch1 = (a.k1 + KC - 1) / KC;
  const int nchunks = nch1 + (a.k2 + KC - 1) / KC;
  const bool bvec4 = !WFORM && ((a.ldb & 3) == 0) && ((a.Nc & 3) == 0) &&
                     ((reinterpret_cast<uintptr_t>(a.bt) & 15) == 0);
  const uint64_t seed = a.seed_ptr ? (*a.seed_ptr) * 0x9E3779B97F4A7C15ull + a.seed : a.seed;

  floatx16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

  const int foff = (lane & 31) * P + 4 * (lane >> 5);
  auto compute = [&](const float* Ab, const float* Bb, int c) {
    const int klen = c < nch1 ? min(KC, a.k1 - c * KC) : min(KC, a.k2 - (c - nch1) * KC);
    const int ng = (klen + 7) >> 3;
    const float* Af = Ab + wave * 32 * P + foff;
    const float* Bf = Bb + foff;
#pragma unroll
    for (int g = 0; g < KC / 8; ++g) {
      if (g < ng) {
        const float4 av = *reinterpret_cast<const float4*>(Af + 8 * g);
        float4 bv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) bv[t] = *reinterpret_cast<const float4*>(Bf + t * 32 * P + 8 * g);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv[t].x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv[t].y, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv[t].z, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv[t].w, acc[t], 0, 0, 0);
      }
    }
  };

  // one register stage: chunk c + 1's loads are in flight across chunk c's MFMAs
  NT2Stage<AVEC, BVEC, WFORM> st;
  st.load(a, 0, m0, n0, bvec4);
  st.store(a, 0, m0, n0, As[0], Bs[0]);
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) st.load(a, c + 1, m0, n0, bvec4);
    compute(As[buf], Bs[buf], c);
    if (c + 1 < nchunks) st.store(a, c + 1, m0, n0, As[buf ^ 1], Bs[buf ^ 1]);
    __syncthreads();
  }
  nt_epilogue(a, acc, m0, n0, lane, wave, seed);
}

// ------------------------------------------------------------------------------------ TN

// slab layout: dW[Nr][Kc] | db[Nr] | dW2[nproj][Nr] | dzsum[nproj]
//
// Structure (per 512-thread block, rows [mbeg, mend)): chunks of MC=32 rows, double-buffered
// through LDS.  While the MFMAs of chunk c run, chunk c+1's operands are already in flight
// into registers (every load unconditional on a clamped row: no branch-around-load waits);
// they are transformed (G prologue) and stored after the MFMAs, then one barrier.
template <int MC, int NTL>
__device__ __forceinline__ void tn_mma(floatx16 (&acc)[KT_PER_WAVE], const float* gptr, const float* aptr, int kt0) {
#pragma unroll 2
  for (int s = 0; s < MC / 2; ++s) {
    const float gf = gptr[2 * s * 128];
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
      const float af = aptr[2 * s * TN_APITCH + (kt0 + t) * 32];
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(gf, af, acc[t], 0, 0, 0);
    }
  }
}

template <bool PROJ, bool MASK, int AVEC, int MC>
__global__ __launch_bounds__(TN_THREADS) void gemm_tn_kernel(TNArgs a) {
  __shared__ __attribute__((aligned(16))) float Gs[2][MC * 128];
  __shared__ __attribute__((aligned(16))) float As[2][MC * TN_APITCH];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int ntile = wave & 3;
  const int kt0 = (wave >> 2) * KT_PER_WAVE;
  const int Kc = a.k1 + a.k2;
  const int nkt = (Kc + 31) / 32;
  const int ntl = max(0, min(KT_PER_WAVE, nkt - kt0));
  const int64_t mbeg = (int64_t)blockIdx.x * a.rows_per_block;
  const int64_t mend = min(a.M, mbeg + a.rows_per_block);

  floatx16 acc[KT_PER_WAVE];
#pragma unroll
  for (int t = 0; t < KT_PER_WAVE; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

  const int pn = tid & 127;  // prologue: column pn, rows rg*GR .. rg*GR+GR-1
  const int rg = tid >> 7;
  const bool colok = pn < a.Nr;
  const int pnc = colok ? pn : 0;
  float db = 0.0f;
  float dw2[MAXPROJ] = {0.f, 0.f, 0.f, 0.f};
  float dzs = 0.f;  // column pn's dz sum (pn < MAXPROJ only)
  __shared__ float Ps[MAXPROJ * 128];  // projection columns (kept in LDS: saves 4 VGPRs per thread)
  if constexpr (PROJ) {
    if (tid < 128) {
#pragma unroll
      for (int q = 0; q < MAXPROJ; ++q) Ps[q * 128 + tid] = (q < a.nproj && tid < a.Nr) ? a.proj[q * a.Nr + tid] : 0.0f;
    }
    __syncthreads();  // Ps is read by every thread's first store_chunk
  }
  constexpr int NRG = TN_THREADS / 128;              // prologue row groups
  constexpr int GR = MC / NRG;                       // prologue rows per thread
  // A staging: 32 threads per chunk row; thread owns columns (tl*AVEC + 32*AVEC*j), j < AJ
  constexpr int TPR = TN_THREADS / MC;               // threads per row (32)
  constexpr int AJ = KMAX / (TPR * AVEC);            // vectors per thread per row
  const int ar = tid / TPR;                          // this thread's chunk row
  const int tl = tid - ar * TPR;
  float rg_in[GR][PROJ ? MAXPROJ : 1];
  float rh[GR];
  float ra[AJ][AVEC];

  auto load_chunk = [&](int64_t m0) {
#pragma unroll
    for (int i = 0; i < GR; ++i) {
      int64_t m = m0 + rg * GR + i;
      m = m < mend ? m : mend - 1;  // clamped: always a valid row, masked in store_chunk
      if constexpr (PROJ) {
        if (a.nproj == 4 && (a.lddz & 3) == 0 && (reinterpret_cast<uintptr_t>(a.dz) & 15) == 0) {
          float4 t = *reinterpret_cast<const float4*>(a.dz + m * a.lddz);
          rg_in[i][0] = t.x; rg_in[i][1] = t.y; rg_in[i][2] = t.z; rg_in[i][3] = t.w;
        } else {
#pragma unroll
          for (int q = 0; q < MAXPROJ; ++q) rg_in[i][q] = a.dz[m * a.lddz + (q < a.nproj ? q : 0)];
        }
      } else {
        rg_in[i][0] = a.g[m * a.ldg + pnc];
      }
      if constexpr (MASK) rh[i] = a.h[m * a.ldh + pnc];
    }
    int64_t m = m0 + ar;
    m = m < mend ? m : mend - 1;
    const float* b1 = a.a1 + m * a.lda1;
    const float* b2 = a.a2 + m * a.lda2 - a.k1;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int k = tl * AVEC + TPR * AVEC * j;
      const float* src = k < a.k1 ? b1 + k : (k < Kc ? b2 + k : b1);
      if constexpr (AVEC == 2) {
        float2 t = *reinterpret_cast<const float2*>(src);
        ra[j][0] = t.x; ra[j][1] = t.y;
      } else {
        ra[j][0] = *src;
      }
    }
  };

  auto store_chunk = [&](int64_t m0, int buf) {
#pragma unroll
    for (int i = 0; i < GR; ++i) {
      const int r = rg * GR + i;
      const bool rok = m0 + r < mend;
      const bool ok = rok && colok;
      float g;
      if constexpr (PROJ) {
        g = rg_in[i][0] * Ps[pn];
#pragma unroll
        for (int q = 1; q < MAXPROJ; ++q) g = fmaf(rg_in[i][q], Ps[q * 128 + pn], g);
      } else {
        g = rg_in[i][0];
      }
      if constexpr (MASK) {
        g = rh[i] > 0.0f ? g * a.hscale : 0.0f;
        if constexpr (PROJ) {
#pragma unroll
          for (int q = 0; q < MAXPROJ; ++q) dw2[q] = fmaf(ok ? rg_in[i][q] : 0.0f, rh[i], dw2[q]);
        }
      }
      if constexpr (PROJ) {
        if (pn < MAXPROJ) dzs += rok ? rg_in[i][pn] : 0.0f;  // lanes 0..3 of each row group own one dz column
      }
      g = ok ? g : 0.0f;
      db += g;
      if (a.gout && ok) a.gout[(m0 + r) * a.ldgout + pn] = g;
      Gs[buf][r * 128 + pn] = g;
    }
    const bool rok = m0 + ar < mend;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int k = tl * AVEC + TPR * AVEC * j;
      const bool ok = rok && k < Kc;
      if constexpr (AVEC == 2) {
        *reinterpret_cast<float2*>(&As[buf][ar * TN_APITCH + k]) = make_float2(ok ? ra[j][0] : 0.0f, ok ? ra[j][1] : 0.0f);
      } else {
        As[buf][ar * TN_APITCH + k] = ok ? ra[j][0] : 0.0f;
      }
    }
  };

  if (mbeg < mend) {
    load_chunk(mbeg);
    store_chunk(mbeg, 0);
    __syncthreads();
    int buf = 0;
    for (int64_t m0 = mbeg; m0 < mend; m0 += MC) {
      const bool more = m0 + MC < mend;
      if (more) load_chunk(m0 + MC);
      const float* gptr = Gs[buf] + (lane >> 5) * 128 + ntile * 32 + (lane & 31);
      const float* aptr = As[buf] + (lane >> 5) * TN_APITCH + (lane & 31);
      switch (ntl) {
        case 3: tn_mma<MC, 3>(acc, gptr, aptr, kt0); break;
        case 2: tn_mma<MC, 2>(acc, gptr, aptr, kt0); break;
        case 1: tn_mma<MC, 1>(acc, gptr, aptr, kt0); break;
        default: break;
      }
      if (more) store_chunk(m0 + MC, buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  // ---- write this block's partial dW
  float* slab = a.slab + (int64_t)blockIdx.x * a.slab_stride;
#pragma unroll
  for (int t = 0; t < KT_PER_WAVE; ++t) {
    const int kt = kt0 + t;
    if (kt >= nkt) continue;
    const int col = kt * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ntile * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      // segment-major: dW1 = [Nr][k1] then dW2 = [Nr][k2], each contiguous
      const int64_t idx = col < a.k1 ? (int64_t)row * a.k1 + col
                                     : (int64_t)a.Nr * a.k1 + (int64_t)row * a.k2 + (col - a.k1);
      if (row < a.Nr && col < Kc) slab[idx] = acc[t][r];
    }
  }
  // ---- side sums: reduce the 4 row groups through LDS (fixed order); reuse Gs as scratch
  float* red = &As[0][0];  // 2*MC*KMAX >= NRG*128*(1+MAXPROJ) floats for MC >= 16
  static_assert(2 * MC * TN_APITCH >= (TN_THREADS / 128) * 128 * (1 + MAXPROJ), "side-sum scratch");
  constexpr int ns = 1 + MAXPROJ;
  __syncthreads();
  red[(rg * 128 + pn) * ns + 0] = db;
#pragma unroll
  for (int q = 0; q < MAXPROJ; ++q) red[(rg * 128 + pn) * ns + 1 + q] = dw2[q];
  __syncthreads();
  if (tid < 128 && colok) {
    float* side = slab + (int64_t)a.Nr * Kc;
    float s2 = 0.f;
    for (int g2 = 0; g2 < NRG; ++g2) s2 += red[(g2 * 128 + pn) * ns];
    side[pn] = s2;
    for (int q = 0; q < a.nproj; ++q) {
      float w = 0.f;
      for (int g2 = 0; g2 < NRG; ++g2) w += red[(g2 * 128 + pn) * ns + 1 + q];
      side[a.Nr + q * a.Nr + pn] = w;
    }
  }
  __syncthreads();
  if (pn < MAXPROJ) red[rg * MAXPROJ + pn] = dzs;
  __syncthreads();
  if (tid < a.nproj) {
    float s2 = 0.f;
    for (int g2 = 0; g2 < NRG; ++g2) s2 += red[g2 * MAXPROJ + tid];
    slab[(int64_t)a.Nr * Kc + a.Nr + a.nproj * a.Nr + tid] = s2;
  }
}

// out[j] = Σ_b slab[b][j], deterministic.  A 256-thread block owns 16 float4 outputs; its 16
// thread rows each sum a fixed 1/16 of the slabs (4 independent loads in flight), and the 16
// partials are combined through LDS in slab order.  ~700 blocks: the whole chip streams the
// slabs instead of one thread per output walking all of them.
// SqOut (ABI 20): the clip + Adam norm partials of this block's outputs (Σ out² and the count of
// non-finite outputs, outside [skip_lo, skip_hi)), and block 0 snapshots the optimizer's step count.
struct SqOut {
  float* part; const float* step; int64_t skip_lo, skip_hi;
};
constexpr int kRedGrp = 16;
// EMPTY: the slabs carry the flag-driven TN's empty word (an instantiation of its own: the plain
// form keeps its registers)
template <bool EMPTY>
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slab, int64_t stride, int nblk,
                                                          float* __restrict__ out, int64_t n, SqOut sq = SqOut{}) {
  __shared__ float4 part[kRedGrp][kRedOut];
  const int o = threadIdx.x & (kRedOut - 1);
  const int g = threadIdx.x / kRedOut;
  const int64_t j = ((int64_t)blockIdx.x * kRedOut + o) * 4;
  const int per = (nblk + kRedGrp - 1) / kRedGrp;
  const int b0 = g * per, b1 = min(nblk, b0 + per);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (j < n && EMPTY) {
    // the flag-driven TN's slabs: the last word of a slab is 1 where its row block wrote nothing
    // else (TNArgs::slab_empty).  Such a slab is not read — its memory is stale — and nothing is
    // added for it: it would have held +0.0f everywhere, and s starts at +0.0f and never becomes
    // -0.0f (x + y is -0.0f only for two negative zeros), so s + (+0.0f) == s bit for bit.  The
    // group's slabs are still added in order; 16 at a time have their words, then their loads, in
    // flight together.
    for (int bb = b0; bb < b1; bb += 16) {
      uint32_t live = 0;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(slab)[(int64_t)min(bb + u, b1 - 1) * stride + stride - 1];
        live |= (bb + u < b1 && w == 0u) ? 1u << u : 0u;
      }
      float4 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (live >> u & 1) v[u] = *reinterpret_cast<const float4*>(slab + (int64_t)(bb + u) * stride + j);
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (live >> u & 1) {
          s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w;
        }
    }
  } else if (j < n) {
    int b = b0;
    for (; b + 4 <= b1; b += 4) {
      float4 v0 = *reinterpret_cast<const float4*>(slab + (int64_t)(b + 0) * stride + j);
      float4 v1 = *reinterpret_cast<const float4*>(slab + (int64_t)(b + 1) * stride + j);
      float4 v2 = *reinterpret_cast<const float4*>(slab + (int64_t)(b + 2) * stride + j);
      float4 v3 = *reinterpret_cast<const float4*>(slab + (int64_t)(b + 3) * stride + j);
      s.x = (((s.x + v0.x) + v1.x) + v2.x) + v3.x;
      s.y = (((s.y + v0.y) + v1.y) + v2.y) + v3.y;
      s.z = (((s.z + v0.z) + v1.z) + v2.z) + v3.z;
      s.w = (((s.w + v0.w) + v1.w) + v2.w) + v3.w;
    }
    for (; b < b1; ++b) {
      float4 v = *reinterpret_cast<const float4*>(slab + (int64_t)b * stride + j);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  part[g][o] = s;
  __syncthreads();
  if (g != 0) return;  // threads 0..15 (wave 0) finish the block's 16 float4 outputs
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (j < n) {
    t = part[0][o];
    for (int q = 1; q < kRedGrp; ++q) {
      float4 v = part[q][o];
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    if (j + 0 < n) out[j + 0] = t.x;
    if (j + 1 < n) out[j + 1] = t.y;
    if (j + 2 < n) out[j + 2] = t.z;
    if (j + 3 < n) out[j + 3] = t.w;
  }
  if (sq.part) {  // this block's norm partials: its 64 outputs in a fixed order (ABI 20)
    float s2 = 0.f, nf = 0.f;
    const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t je = j + e;
      const bool use = je < n && (je < sq.skip_lo || je >= sq.skip_hi);
      s2 = use ? fmaf(tv[e], tv[e], s2) : s2;
      nf += (use && !isfinite(tv[e])) ? 1.f : 0.f;
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
      s2 += __shfl_xor(s2, off, 16);
      nf += __shfl_xor(nf, off, 16);
    }
    if (o == 0) {
      sq.part[blockIdx.x] = s2;
      sq.part[gridDim.x + blockIdx.x] = nf;
      if (blockIdx.x == 0) sq.part[2 * gridDim.x] = sq.step[0];
    }
  }
}


}  // namespace

// The exact-f32 NT (avec: widest A row vector; a.wvec: widest W row vector; no w1: the Bt form).
void launch_nt_f32(const NTArgs& a, int avec, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(a.M, NT_BM), (unsigned)ceil_div(a.Nc, BN));
  const int bvec = !a.w1 ? 0 : a.wvec == 4 ? 4 : a.wvec == 2 ? 2 : 1;
  with_rung<1, 2, 4>(avec == 4 ? 4 : avec == 2 ? 2 : 1, [&](auto av) {
    with_rung<0, 1, 2, 4>(bvec, [&](auto bv) {
      gemm_nt2_kernel<av(), (bv() ? bv() : 1), (bv() != 0)><<<grid, 256, 0, st>>>(a);
    });
  });
}

void launch_tn_f32(const TNArgs& a, int nblk, hipStream_t st) {
  const bool v2 = (a.k1 % 2 == 0) && (a.lda1 % 2 == 0) && aligned(a.a1, 8) &&
                  (a.k2 == 0 || ((a.k2 % 2 == 0) && (a.lda2 % 2 == 0) && aligned(a.a2, 8)));
  tn_forms(a, [&](auto proj, auto mask, auto) {
    // the dz·P + mask prologue holds twice the staging registers: 16-row chunks keep it spill-free
    constexpr int MC = (proj() && mask()) ? 16 : 32;
    if (v2) gemm_tn_kernel<proj(), mask(), 2, MC><<<nblk, TN_THREADS, 0, st>>>(a);
    else gemm_tn_kernel<proj(), mask(), 1, MC><<<nblk, TN_THREADS, 0, st>>>(a);
  });
}

void launch_slab_reduce(const float* slab, int64_t stride, int nred, float* out, int64_t n_out,
                        const gnn_gemm_tn_params* sq, hipStream_t st, bool empty) {
  const SqOut sqo = sq && sq->sq_partial ? SqOut{sq->sq_partial, sq->sq_step, sq->sq_skip_lo, sq->sq_skip_hi} : SqOut{};
  const unsigned nb = (unsigned)ceil_div(ceil_div(n_out, 4), kRedOut);
  if (empty) slab_reduce_kernel<true><<<nb, 256, 0, st>>>(slab, stride, nred, out, n_out, sqo);
  else slab_reduce_kernel<false><<<nb, 256, 0, st>>>(slab, stride, nred, out, n_out, sqo);
}

}  // namespace gnnmp
