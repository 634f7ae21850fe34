// K14 — ranking metrics on the device: average precision (sklearn's average_precision_score, the
// reference's pr_auc_illicit, src/utils/metrics.py:10-12), segmented average precision (the
// per-timestep loop of src/train_gnn.py:497-519), precision@k (metrics.py:37-39) and the
// per-replicate metrics of the paired bootstrap (src/analysis/bootstrap_compare.py).
//
// Rank plan: ONE stable rocPRIM radix sort of (segment, ~orderable(score)) keys with the element
// index as value gives the order (segment ascending, score descending, index ascending); a flags
// pass marks tie-group ends / group starts / segment starts and writes seg_ptr and the inverse
// permutation.  Excluded elements carry pseudo-segment S and sort behind everything.
//
// Average precision over the order: a two-level segmented scan of integer (TP, FP, TP-in-group)
// triples — per-block aggregates, one block scanning the aggregates into per-block carries, then
// the blocks again with their carry — and, at every group end g, the f64 term
// (TP_g - TP_{g-1}) · TP_g / (TP_g + FP_g).  The terms are summed per thread chunk, wave, block
// (a segmented f64 scan in one fixed tree) and finally block partials in block order by one
// thread per segment; AP = Σ / P.  No float atomics anywhere: two runs give the same bits.
//
// Bootstrap: a replicate is a vector of integer weights (how often each sample was drawn).  One
// workgroup per (replicate, run) histograms the drawn indices into RANK space with integer
// atomics (LDS up to GNN_RANK_BOOT_LDS_MAX_N elements, a global [Bc, 2, n] count buffer filled
// by a launch of its own above that) and runs the weighted scan over the counts.
#include <rocprim/device/device_radix_sort.hpp>

#include "common.hpp"
#include "rank_scan.hpp"

namespace gnnmp {
namespace {

constexpr int kTB = 256;                        // threads of the scan blocks
constexpr int kItems = 4;                       // consecutive order positions per thread
constexpr int kTile = GNN_RANK_TILE;            // positions per block
static_assert(kTB * kItems == kTile, "GNN_RANK_TILE is the scan blocks' tile");
constexpr int kBootTB = 1024;                   // threads of a bootstrap workgroup
constexpr int kBootLdsN = GNN_RANK_BOOT_LDS_MAX_N;
constexpr int kBootLdsWords = kBootLdsN + kBootLdsN / 32;  // one pad word per 32 (chunked walks hit all banks)
static_assert((size_t)kBootLdsWords * 4 + 4096 <= 160 * 1024, "the LDS histogram must fit one CU's 160 KiB");

// ------------------------------------------------------------------------ scan states
struct Cnt {  // segmented counts: tp/fp since the last segment start, gtp since the last group start
  int32_t seg, grp, tp, fp, gtp;
};
struct CntOp {
  __device__ __forceinline__ Cnt operator()(const Cnt& a, const Cnt& b) const {
    Cnt r;
    r.seg = a.seg | b.seg;
    r.grp = a.grp | b.grp;
    r.tp = b.seg ? b.tp : a.tp + b.tp;
    r.fp = b.seg ? b.fp : a.fp + b.fp;
    r.gtp = b.grp ? b.gtp : a.gtp + b.gtp;
    return r;
  }
};
struct Part {  // segmented sums: AP terms (f64, fixed tree) and P@k hits since the last segment start
  double sum;
  long long hits;
  int32_t seg, pad;
};
struct PartOp {
  __device__ __forceinline__ Part operator()(const Part& a, const Part& b) const {
    Part r;
    r.seg = a.seg | b.seg;
    r.pad = 0;
    r.sum = b.seg ? b.sum : a.sum + b.sum;
    r.hits = b.seg ? b.hits : a.hits + b.hits;
    return r;
  }
};
static_assert(sizeof(Cnt) == 20 && sizeof(Part) == 24, "scan states move between lanes as 32-bit words");

// ------------------------------------------------------------------------ rank plan
// Orderable image of a score, inverted: ascending key = descending score.  -0.0 counts as +0.0.
__device__ __forceinline__ uint32_t desc_key(float s, bool* is_nan) {
  uint32_t u = __float_as_uint(s);
  *is_nan = (u & 0x7fffffffu) > 0x7f800000u;
  if (u == 0x80000000u) u = 0u;
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return ~u;
}

__global__ void rank_keys_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ include,
                                 const int32_t* __restrict__ segment, int64_t n, int64_t S,
                                 uint64_t* __restrict__ keys, int32_t* __restrict__ vals,
                                 int32_t* __restrict__ status) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool inc = include ? include[i] != 0 : true;
  const int64_t seg = segment ? (int64_t)segment[i] : 0;
  if (inc && (seg < 0 || seg >= S)) {
    atomicOr(status, GNN_RANK_STATUS_SEGMENT);
    inc = false;
  }
  bool is_nan;
  const uint32_t k = desc_key(scores[i], &is_nan);
  if (inc && is_nan) atomicOr(status, GNN_RANK_STATUS_NAN);
  keys[i] = ((uint64_t)(inc ? seg : S) << 32) | k;
  vals[i] = (int32_t)i;
}

// Over the sorted keys, t in [0, n]: flags[t], rank[order[t]] = t, and seg_ptr[i] = first position
// whose segment is >= i (i in [0, S]; seg_ptr[S] = m, the number of included elements).
__global__ void rank_flags_kernel(const uint64_t* __restrict__ key, const int32_t* __restrict__ order, int64_t n,
                                  int64_t S, uint8_t* __restrict__ flags, int32_t* __restrict__ seg_ptr,
                                  int32_t* __restrict__ rank) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t > n) return;
  const uint64_t cur = t < n ? key[t] : ((uint64_t)S << 32);
  const int64_t cseg = t < n ? (int64_t)(cur >> 32) : S;
  const bool first = t == 0;
  const uint64_t prev = first ? 0 : key[t - 1];
  const int64_t pseg = first ? -1 : (int64_t)(prev >> 32);
  for (int64_t i = pseg + 1; i <= cseg && i <= S; ++i) seg_ptr[i] = (int32_t)t;
  if (t == n) return;
  const bool gstart = first || prev != cur;
  const bool gend = t == n - 1 || key[t + 1] != cur;
  flags[t] = (uint8_t)((gend ? kGroupEnd : 0) | (pseg != cseg ? kSegStart : 0) | (gstart ? kGroupStart : 0));
  if (rank) rank[order[t]] = (int32_t)t;
}

unsigned bits_for(int64_t v) {  // bits needed to hold values 0..v
  unsigned b = 1;
  while (b < 31 && (int64_t(1) << b) <= v) ++b;
  return b;
}

gnn_status rank_sort_bytes(int64_t n, size_t* bytes) {
  size_t tb = 0;
  hipError_t err = rocprim::radix_sort_pairs(nullptr, tb, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr,
                                             (int32_t*)nullptr, (size_t)(n > 0 ? n : 1), 0, 64, (hipStream_t)0);
  if (err != hipSuccess) return hip_check(err, "rank_sort_bytes");
  *bytes = tb;
  return GNN_OK;
}

struct PlanLayout {
  uint64_t *key_in, *key_out;
  int32_t* val_in;
  void* sort_tmp;
};

template <typename C>
void carve_plan(C& c, int64_t n, size_t sort_bytes, PlanLayout* L) {
  const size_t n1 = (size_t)(n > 0 ? n : 1);
  auto a = c.template take<uint64_t>(n1);
  auto b = c.template take<uint64_t>(n1);
  auto v = c.template take<int32_t>(n1);
  auto s = c.template take<char>(sort_bytes);
  if (L) {
    L->key_in = a; L->key_out = b; L->val_in = v; L->sort_tmp = (void*)s;
  }
}

struct SizerAdapter {
  WorkspaceSizer s;
  template <typename T>
  T* take(size_t n) { s.take<T>(n); return nullptr; }
};

// ------------------------------------------------------------------------ segmented AP / P@k
__device__ __forceinline__ int32_t find_seg(const int32_t* __restrict__ seg_ptr, int64_t S, int64_t t) {
  int64_t lo = 0, hi = S;  // largest s in [0, S) with seg_ptr[s] <= t (empty segments repeat a pointer)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (seg_ptr[mid] <= t) lo = mid; else hi = mid;
  }
  return (int32_t)lo;
}

// A thread's kItems positions: element states (inclusive within the thread), own flags, the flag
// of the following position (kSegStart past the end) and labels.
struct TileLoad {
  Cnt e[kItems];
  uint8_t fl[kItems], nfl[kItems], y[kItems];
};

__device__ __forceinline__ void load_tile(const int32_t* __restrict__ order, const uint8_t* __restrict__ flags,
                                          const uint8_t* __restrict__ pos, int64_t m, int64_t base, TileLoad& L) {
  const CntOp op;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int64_t t = base + j;
    if (t < m) {
      const uint8_t f = flags[t];
      const uint8_t y = pos[order[t]] != 0;
      L.fl[j] = f;
      L.y[j] = y;
      L.e[j] = Cnt{(f & kSegStart) ? 1 : 0, (f & kGroupStart) ? 1 : 0, y, 1 - y, y};
    } else {
      L.fl[j] = 0;
      L.y[j] = 0;
      L.e[j] = Cnt{0, 0, 0, 0, 0};
    }
  }
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int64_t t = base + j + 1;
    L.nfl[j] = j + 1 < kItems ? (t < m ? L.fl[j + 1] : (uint8_t)kSegStart) : (t < m ? flags[t] : (uint8_t)kSegStart);
  }
#pragma unroll
  for (int j = 1; j < kItems; ++j) L.e[j] = op(L.e[j - 1], L.e[j]);
}

__global__ __launch_bounds__(kTB) void ap_aggregate_kernel(const int32_t* __restrict__ order,
                                                           const uint8_t* __restrict__ flags,
                                                           const int32_t* __restrict__ seg_ptr,
                                                           const uint8_t* __restrict__ pos, int64_t S,
                                                           Cnt* __restrict__ agg) {
  __shared__ Cnt wt[kTB / kWave];
  const int64_t m = seg_ptr[S];
  TileLoad L;
  load_tile(order, flags, pos, m, blockIdx.x * (int64_t)kTile + threadIdx.x * kItems, L);
  Cnt ex, tot;
  block_scan<kTB / kWave>(L.e[kItems - 1], CntOp(), Cnt{0, 0, 0, 0, 0}, wt, &ex, &tot);
  if (threadIdx.x == 0) agg[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kTB) void ap_carry_kernel(const Cnt* __restrict__ agg, int64_t nb,
                                                       Cnt* __restrict__ carry) {
  __shared__ Cnt wt[kTB / kWave];
  const CntOp op;
  const Cnt ident{0, 0, 0, 0, 0};
  Cnt run = ident;
  for (int64_t b0 = 0; b0 < nb; b0 += kTB) {
    const int64_t b = b0 + threadIdx.x;
    Cnt ex, tot;
    block_scan<kTB / kWave>(b < nb ? agg[b] : ident, op, ident, wt, &ex, &tot);
    if (b < nb) carry[b] = op(run, ex);
    run = op(run, tot);
  }
}

__global__ __launch_bounds__(kTB) void ap_terms_kernel(const int32_t* __restrict__ order,
                                                       const uint8_t* __restrict__ flags,
                                                       const int32_t* __restrict__ seg_ptr,
                                                       const uint8_t* __restrict__ pos, int64_t S, int64_t k,
                                                       const Cnt* __restrict__ carry, Part* __restrict__ head_part,
                                                       Part* __restrict__ first_part, int64_t* __restrict__ P,
                                                       int64_t* __restrict__ cnt) {
  __shared__ Cnt wt[kTB / kWave];
  __shared__ Part wp[kTB / kWave];
  const CntOp op;
  const PartOp pop;
  const int64_t m = seg_ptr[S];
  const int64_t base = blockIdx.x * (int64_t)kTile + threadIdx.x * kItems;
  TileLoad L;
  load_tile(order, flags, pos, m, base, L);
  Cnt ex, tot;
  block_scan<kTB / kWave>(L.e[kItems - 1], op, Cnt{0, 0, 0, 0, 0}, wt, &ex, &tot);
  ex = op(carry[blockIdx.x], ex);
  Cnt c[kItems];
  Part p[kItems];
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    c[j] = op(ex, L.e[j]);
    const bool valid = base + j < m;
    const int32_t seen = c[j].tp + c[j].fp;  // >= 1 for a valid element
    const double term = (valid && (L.fl[j] & kGroupEnd))
                            ? (double)c[j].gtp * ((double)c[j].tp / (double)seen) : 0.0;
    const long long hit = (valid && k > 0 && (int64_t)seen - 1 < k) ? L.y[j] : 0;
    p[j] = Part{term, hit, (L.fl[j] & kSegStart) ? 1 : 0, 0};
  }
#pragma unroll
  for (int j = 1; j < kItems; ++j) p[j] = pop(p[j - 1], p[j]);
  Part pex, ptot;
  block_scan<kTB / kWave>(p[kItems - 1], pop, Part{0.0, 0, 0, 0}, wp, &pex, &ptot);
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int64_t t = base + j;
    if (t >= m) continue;
    const bool seg_last = (L.nfl[j] & kSegStart) != 0;
    const bool tile_last = (t + 1) % kTile == 0;
    if (!seg_last && !tile_last) continue;
    const Part q = pop(pex, p[j]);
    const int32_t s = find_seg(seg_ptr, S, t);
    // q sums from the segment's start if that lies in this tile (the segment's first partial),
    // else from the tile's start (this block's share of a segment opened by an earlier block)
    if (q.seg) first_part[s] = q;
    else head_part[blockIdx.x] = q;
    if (seg_last) {
      P[s] = c[j].tp;
      cnt[s] = (int64_t)c[j].tp + c[j].fp;
    }
  }
}

__global__ void ap_finish_kernel(const int32_t* __restrict__ seg_ptr, int64_t S, int64_t k,
                                 const Part* __restrict__ head_part, const Part* __restrict__ first_part,
                                 double* __restrict__ ap, int64_t* __restrict__ P, int64_t* __restrict__ cnt,
                                 double* __restrict__ patk) {
  const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int64_t lo = seg_ptr[s], hi = seg_ptr[s + 1];
  if (hi <= lo) {
    ap[s] = 0.0;
    P[s] = 0;
    cnt[s] = 0;
    if (patk) patk[s] = 0.0;
    return;
  }
  double sum = first_part[s].sum;
  long long hits = first_part[s].hits;
  for (int64_t b = lo / kTile + 1; b <= (hi - 1) / kTile; ++b) {  // later blocks' shares, in block order
    sum += head_part[b].sum;
    hits += head_part[b].hits;
  }
  const int64_t p = P[s];
  ap[s] = p > 0 ? sum / (double)p : 0.0;
  if (patk) patk[s] = (double)hits / (double)(k < cnt[s] ? k : cnt[s]);
}

// ------------------------------------------------------------------------ bootstrap
__device__ __forceinline__ int lds_slot(int r) { return r + (r >> 5); }

__global__ void boot_hist_kernel(const int32_t* __restrict__ rank_a, const int32_t* __restrict__ rank_b,
                                 const int32_t* __restrict__ idx, int64_t n, int32_t* __restrict__ counts,
                                 int32_t* __restrict__ status) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t rep = blockIdx.y, run = blockIdx.z;
  const int32_t i = idx[rep * n + j];
  if (i < 0 || i >= n) {
    atomicOr(status, GNN_RANK_STATUS_INDEX);
    return;
  }
  const int32_t r = (run ? rank_b : rank_a)[i];
  if (r < 0 || r >= n) {
    atomicOr(status, GNN_RANK_STATUS_INDEX);
    return;
  }
  atomicAdd(&counts[(rep * 2 + run) * n + r], 1);
}

// One workgroup per (replicate, run): weights w[r] = draws of the sample at rank r, then the
// weighted AP / P@k walk.  Thread t owns the contiguous ranks [t·C, (t+1)·C), C = ceil(n / 1024):
// pass 1 folds them into one state, a block scan gives every thread its prefix, pass 2 walks them
// again with the prefix and sums the terms; thread partials combine wave by wave in one order.
template <bool LDS>
__global__ __launch_bounds__(kBootTB) void boot_scan_kernel(
    const int32_t* __restrict__ order_a, const int32_t* __restrict__ rank_a, const uint8_t* __restrict__ flags_a,
    const int32_t* __restrict__ order_b, const int32_t* __restrict__ rank_b, const uint8_t* __restrict__ flags_b,
    const uint8_t* __restrict__ pos, const int32_t* __restrict__ idx, int64_t n, int64_t k,
    const int32_t* __restrict__ counts, double* __restrict__ ap_a, double* __restrict__ ap_b,
    double* __restrict__ patk_a, double* __restrict__ patk_b, int32_t* __restrict__ status) {
  constexpr int NW = kBootTB / kWave;
  __shared__ Cnt wt[NW];
  __shared__ Part wp[NW];
  const int64_t rep = blockIdx.x;
  const int run = blockIdx.y;
  const int32_t* order = run ? order_b : order_a;
  const uint8_t* flags = run ? flags_b : flags_a;
  const int32_t* w_glob = nullptr;
  int32_t* hist = nullptr;
  if constexpr (LDS) {
    __shared__ int32_t hist_lds[kBootLdsWords];
    hist = hist_lds;
    const int32_t* rank = run ? rank_b : rank_a;
    const int words = lds_slot((int)n - 1) + 1;
    for (int i = threadIdx.x; i < words; i += kBootTB) hist[i] = 0;
    __syncthreads();
    for (int64_t j = threadIdx.x; j < n; j += kBootTB) {
      const int32_t i = idx[rep * n + j];
      const int32_t r = (i >= 0 && i < n) ? rank[i] : -1;
      if (r < 0 || r >= n) atomicOr(status, GNN_RANK_STATUS_INDEX);
      else atomicAdd(&hist[lds_slot(r)], 1);
    }
    __syncthreads();
  } else {
    w_glob = counts + (rep * 2 + run) * n;
  }
  auto weight = [&](int64_t r) -> int32_t {
    if constexpr (LDS) return hist[lds_slot((int)r)];
    else return w_glob[r];
  };
  const CntOp op;
  const Cnt ident{0, 0, 0, 0, 0};
  const int64_t C = (n + kBootTB - 1) / kBootTB;
  const int64_t r0 = threadIdx.x * C < n ? threadIdx.x * C : n;
  const int64_t r1 = r0 + C < n ? r0 + C : n;
  Cnt mine = ident;
  for (int64_t r = r0; r < r1; ++r) {
    const int32_t w = weight(r);
    const int32_t wy = pos[order[r]] ? w : 0;
    mine = op(mine, Cnt{0, (flags[r] & kGroupStart) ? 1 : 0, wy, w - wy, wy});
  }
  Cnt run_c, tot;
  block_scan<NW>(mine, op, ident, wt, &run_c, &tot);
  double sum = 0.0;
  long long hits = 0;
  for (int64_t r = r0; r < r1; ++r) {
    const int32_t w = weight(r);
    const int32_t wy = pos[order[r]] ? w : 0;
    const uint8_t f = flags[r];
    run_c = op(run_c, Cnt{0, (f & kGroupStart) ? 1 : 0, wy, w - wy, wy});
    if ((f & kGroupEnd) && run_c.gtp > 0)
      sum += (double)run_c.gtp * ((double)run_c.tp / (double)(run_c.tp + run_c.fp));
    const int64_t before = (int64_t)run_c.tp + run_c.fp - w;  // copies ranked ahead of this sample
    if (wy && before < k) hits += (k - before < w) ? k - before : w;
  }
  // thread partials -> block sum: the same segmented tree with no segment start is a plain ordered sum
  Part pex, ptot;
  block_scan<NW>(Part{sum, hits, 0, 0}, PartOp(), Part{0.0, 0, 0, 0}, wp, &pex, &ptot);
  if (threadIdx.x == 0) {
    const int64_t drawn = (int64_t)tot.tp + tot.fp;
    (run ? ap_b : ap_a)[rep] = tot.tp > 0 ? ptot.sum / (double)tot.tp : 0.0;
    (run ? patk_b : patk_a)[rep] = drawn > 0 ? (double)ptot.hits / (double)(k < drawn ? k : drawn) : 0.0;
  }
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" gnn_status gnn_rank_plan_workspace_size(int64_t n, int64_t num_segments, size_t* bytes) {
  if (!bytes || n < 0 || num_segments < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  if (n >= INT32_MAX || num_segments >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n or S exceeds int32 range");
  size_t sb = 0;
  gnn_status s = rank_sort_bytes(n, &sb);
  if (s != GNN_OK) return s;
  SizerAdapter a;
  carve_plan(a, n, sb, nullptr);
  *bytes = a.s.used + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_rank_plan_build(const float* scores, const uint8_t* include, const int32_t* segment,
                                          int64_t n, int64_t num_segments, int32_t* order, uint8_t* flags,
                                          int32_t* seg_ptr, int32_t* rank, int32_t* status, void* workspace,
                                          size_t workspace_bytes, gnn_stream_t stream) {
  const int64_t S = num_segments;
  if (n < 0 || S < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n or S");
  if (n >= INT32_MAX || S >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n or S exceeds int32 range");
  if (!seg_ptr || !status || (n > 0 && (!scores || !order || !flags)))
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  hipStream_t st = (hipStream_t)stream;
  size_t sb = 0;
  gnn_status s = rank_sort_bytes(n, &sb);
  if (s != GNN_OK) return s;
  WorkspaceCarver c(workspace, workspace_bytes);
  PlanLayout L;
  carve_plan(c, n, sb, &L);
  if (!c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  const int TB = 256;
  if (n > 0) {
    rank_keys_kernel<<<ceil_div(n, TB), TB, 0, st>>>(scores, include, segment, n, S, L.key_in, L.val_in, status);
    GNN_LAUNCH_CHECK();
    GNN_HIP_TRY(rocprim::radix_sort_pairs(L.sort_tmp, sb, L.key_in, L.key_out, L.val_in, order, (size_t)n, 0,
                                          32 + bits_for(S), st));
  }
  rank_flags_kernel<<<ceil_div(n + 1, TB), TB, 0, st>>>(L.key_out, order, n, S, flags, seg_ptr, rank);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

namespace {
struct ApLayout {
  Cnt *agg, *carry;
  Part *head, *first;
};
template <typename C>
void carve_ap(C& c, int64_t nb, int64_t S, ApLayout* L) {
  auto a = c.template take<Cnt>((size_t)nb);
  auto b = c.template take<Cnt>((size_t)nb);
  auto h = c.template take<Part>((size_t)nb);
  auto f = c.template take<Part>((size_t)(S > 0 ? S : 1));
  if (L) {
    L->agg = a; L->carry = b; L->head = h; L->first = f;
  }
}
}  // namespace

extern "C" gnn_status gnn_rank_ap_workspace_size(int64_t n, int64_t num_segments, size_t* bytes) {
  if (!bytes || n < 0 || num_segments < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  SizerAdapter a;
  carve_ap(a, ceil_div(n > 0 ? n : 1, kTile), num_segments, nullptr);
  *bytes = a.s.used + 256;
  return GNN_OK;
}

extern "C" gnn_status gnn_rank_ap(const int32_t* order, const uint8_t* flags, const int32_t* seg_ptr,
                                  const uint8_t* positive, int64_t n, int64_t num_segments, int64_t k, double* ap,
                                  int64_t* num_pos, int64_t* count, double* patk, void* workspace,
                                  size_t workspace_bytes, gnn_stream_t stream) {
  const int64_t S = num_segments;
  if (n < 0 || S < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n or S");
  if (n >= INT32_MAX || S >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, __func__, "n or S exceeds int32 range");
  if (patk && k < 1) return fail(GNN_ERR_INVALID_ARG, __func__, "k < 1");
  if (!seg_ptr || (S > 0 && (!ap || !num_pos || !count)) || (n > 0 && (!order || !flags || !positive)))
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  if (S == 0) return GNN_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = ceil_div(n > 0 ? n : 1, kTile);
  WorkspaceCarver c(workspace, workspace_bytes);
  ApLayout L;
  carve_ap(c, nb, S, &L);
  if (!c.ok) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  const int64_t kk = patk ? k : 0;
  if (n > 0) {
    ap_aggregate_kernel<<<nb, kTB, 0, st>>>(order, flags, seg_ptr, positive, S, L.agg);
    GNN_LAUNCH_CHECK();
    ap_carry_kernel<<<1, kTB, 0, st>>>(L.agg, nb, L.carry);
    GNN_LAUNCH_CHECK();
    ap_terms_kernel<<<nb, kTB, 0, st>>>(order, flags, seg_ptr, positive, S, kk, L.carry, L.head, L.first, num_pos,
                                        count);
    GNN_LAUNCH_CHECK();
  }
  ap_finish_kernel<<<ceil_div(S, 256), 256, 0, st>>>(seg_ptr, S, kk, L.head, L.first, ap, num_pos, count, patk);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}

extern "C" gnn_status gnn_rank_bootstrap_workspace_size(int64_t n, int64_t num_replicates, size_t* bytes) {
  if (!bytes || n < 0 || num_replicates < 0)
    return fail(GNN_ERR_INVALID_ARG, __func__, "negative size or null output");
  *bytes = 256 + (n > kBootLdsN ? align_up((size_t)num_replicates * 2 * (size_t)n * sizeof(int32_t), 256) : 0);
  return GNN_OK;
}

extern "C" gnn_status gnn_rank_bootstrap(const int32_t* order_a, const int32_t* rank_a, const uint8_t* flags_a,
                                         const int32_t* order_b, const int32_t* rank_b, const uint8_t* flags_b,
                                         const uint8_t* positive, const int32_t* sample_idx, int64_t n,
                                         int64_t num_replicates, int64_t k, double* ap_a, double* ap_b,
                                         double* patk_a, double* patk_b, int32_t* status, void* workspace,
                                         size_t workspace_bytes, gnn_stream_t stream) {
  const int64_t B = num_replicates;
  if (n < 0 || B < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "negative n or replicate count");
  if (n >= INT32_MAX || B >= 65536) return fail(GNN_ERR_INVALID_ARG, __func__, "n exceeds int32 range or more than 65535 replicates per call");
  if (k < 1) return fail(GNN_ERR_INVALID_ARG, __func__, "k < 1");
  if (!status || (B > 0 && (!ap_a || !ap_b || !patk_a || !patk_b)) ||
      (B > 0 && n > 0 && (!order_a || !rank_a || !flags_a || !order_b || !rank_b || !flags_b || !positive || !sample_idx)))
    return fail(GNN_ERR_INVALID_ARG, __func__, "null buffer");
  if (B == 0) return GNN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (n <= kBootLdsN) {
    boot_scan_kernel<true><<<dim3((unsigned)B, 2), kBootTB, 0, st>>>(order_a, rank_a, flags_a, order_b, rank_b, flags_b,
                                                                     positive, sample_idx, n, k, nullptr, ap_a, ap_b,
                                                                     patk_a, patk_b, status);
    GNN_LAUNCH_CHECK();
    return GNN_OK;
  }
  const size_t need = (size_t)B * 2 * (size_t)n * sizeof(int32_t);
  if (!workspace || workspace_bytes < need) return fail(GNN_ERR_WORKSPACE, __func__, "workspace too small");
  int32_t* counts = (int32_t*)workspace;
  GNN_HIP_TRY(hipMemsetAsync(counts, 0, need, st));
  boot_hist_kernel<<<dim3((unsigned)ceil_div(n, 256), (unsigned)B, 2), 256, 0, st>>>(rank_a, rank_b, sample_idx, n,
                                                                                      counts, status);
  GNN_LAUNCH_CHECK();
  boot_scan_kernel<false><<<dim3((unsigned)B, 2), kBootTB, 0, st>>>(order_a, rank_a, flags_a, order_b, rank_b, flags_b,
                                                                    positive, sample_idx, n, k, counts, ap_a, ap_b,
                                                                    patk_a, patk_b, status);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}
