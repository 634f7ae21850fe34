// Host entry points of the K7 GEMMs: which kernel a call runs, decided once per GEMM.
//   NT: nt_args (params -> NTArgs, validated) -> nt_select (a kernel id or a refusal) -> one launch
//   TN: tn_args (params -> TNArgs, validated) -> tn_plan (kernel id, grid, slabs, row block, how dz's
//       CSC columns and activity flags arrive, or a refusal) -> launch -> the ordered slab reduce
// nt_select and tn_plan launch nothing.  The *_ok predicates, the column-sum and prep queries and
// the workspace sizes read them (or the block functions they use): a routing rule is written once.
// The kernels and their launchers are in gemm_f32.hip, gemm_x3.hip, gemm_ws.hip, gemm_planes.hip
// and gemm_skinny.hip.
#include "common.hpp"

#include <algorithm>
#include <cstdlib>

#include "gemm_common.hpp"

using namespace gnnmp;
using gemm::aligned;

namespace {

bool bad_dtype(int32_t d) { return d != GNN_DTYPE_F32 && d != GNN_DTYPE_BF16; }
bool bad_math(int32_t m) { return m != GNN_MATH_SPLIT_BF16 && m != GNN_MATH_F32 && m != GNN_MATH_HALF_PAIR; }

// The image fields both params structs share.  Without an image they stay zero.
template <typename P, typename A>
void image_args(const P* p, A* a) {
  if (!p->a_planes) return;
  a->ap = static_cast<const uint16_t*>(p->a_planes);
  a->ap_ld = (int32_t)std::min<int64_t>(p->planes_ld, INT32_MAX);
  a->ap_col2 = (int32_t)std::min<int64_t>(p->planes_col2, INT32_MAX);
  a->ap_ps = p->planes_stride;
  a->ap_h2 = p->planes_format == GNN_PLANES_HALF_PAIR;
  a->ap_exp = a->ap_h2 ? p->planes_exp : 0;
}
// ... and their validation: null when the image fields can be taken
template <typename P>
const char* image_args_bad(const P* p) {
  if (!p->a_planes) return nullptr;
  if (p->planes_format != GNN_PLANES_SPLIT_BF16 && p->planes_format != GNN_PLANES_HALF_PAIR) return "bad planes_format";
  if (p->planes_format == GNN_PLANES_HALF_PAIR && (p->planes_exp < -100 || p->planes_exp > 100))
    return "planes_exp outside [-100, 100]";
  return nullptr;
}

// ------------------------------------------------------------------------------------ NT

// The one translation of NT params.  fn: the entry point refusals are reported under; null (the
// predicates, which answer for a shape and have never validated the rest) only fills *a.
gnn_status nt_args(const gnn_gemm_nt_params* p, NTArgs* out, const char* fn) {
  if (!p) return fail(GNN_ERR_INVALID_ARG, fn, "null params");
  NTArgs a{};
  a.M = p->M; a.Nc = (int32_t)p->N;
  a.a1 = p->a1; a.lda1 = p->lda1; a.k1 = (int32_t)p->k1;
  a.a2 = p->a2; a.lda2 = p->lda2; a.k2 = (int32_t)p->k2;
  a.bt = p->bt; a.ldb = p->ldb; a.w1 = p->w1; a.w2 = p->w2; a.ldw1 = p->ldw1; a.ldw2 = p->ldw2; a.c = p->c;
  a.ldc = p->ldc; a.bias = p->bias; a.relu = p->relu;
  a.dropout = p->dropout_p > 0.f;
  a.keep_thresh = (uint32_t)((1.0 - (double)p->dropout_p) * 16777216.0);
  a.drop_scale = a.dropout ? (float)(1.0 / (1.0 - (double)p->dropout_p)) : 1.0f;
  a.seed = p->seed; a.seed_ptr = p->seed_ptr;
  a.proj = p->proj; a.nproj = p->nproj; a.z = p->z; a.ldz = p->ldz;
  a.wvec2 = a.w1 && (a.ldw1 % 2 == 0) && (a.k1 % 2 == 0) && aligned(a.w1, 8) &&
            (a.k2 == 0 || ((a.ldw2 % 2 == 0) && (a.k2 % 2 == 0) && aligned(a.w2, 8)));
  auto wv = [&](int v) {
    return a.w1 && (a.ldw1 % v == 0) && (a.k1 % v == 0) && aligned(a.w1, 4 * v) &&
           (a.k2 == 0 || ((a.ldw2 % v == 0) && (a.k2 % v == 0) && aligned(a.w2, 4 * v)));
  };
  a.wvec = wv(4) ? 4 : (wv(2) ? 2 : 1);
  a.a_bf16 = p->a_dtype == GNN_DTYPE_BF16; a.c_bf16 = p->c_dtype == GNN_DTYPE_BF16;
  a.mask = p->mask; a.ldmask = p->ldmask; a.mask_scale = p->mask_scale;
  image_args(p, &a);
  a.kmask = p->a_planes ? p->keep_mask : nullptr; a.colsum_part = p->colsum_part; a.rowexp = p->row_exp;
  *out = a;
  if (!fn) return GNN_OK;

  const bool planes_only = p->a_planes && !p->a1;  // A given only as a split image
  if (p->M < 0 || p->N < 1 || p->k1 < 1 || p->k2 < 0 || (!p->a1 && !p->a_planes) ||
      (p->k2 > 0 && !p->a2 && !planes_only))
    return fail(GNN_ERR_INVALID_ARG, fn, "bad shapes / null operands");
  if (!p->bt && !(p->w1 && (p->k2 == 0 || p->w2)))
    return fail(GNN_ERR_INVALID_ARG, fn, "need bt or w1 (and w2 when k2 > 0)");
  if (p->w1 && (p->N > BN || p->ldw1 < p->k1 || (p->k2 > 0 && p->ldw2 < p->k2)))
    return fail(GNN_ERR_INVALID_ARG, fn, "w1/w2 form needs N <= 128 and ldw >= k");
  if ((!planes_only && (p->lda1 < p->k1 || (p->k2 > 0 && p->lda2 < p->k2))) || (p->bt && p->ldb < p->N) ||
      (p->c && p->ldc < p->N))
    return fail(GNN_ERR_INVALID_ARG, fn, "bad leading dimensions");
  if (p->nproj < 0 || p->nproj > 4 || (p->nproj > 0 && (p->N > BN || !p->proj || !p->z || p->ldz < p->nproj)))
    return fail(GNN_ERR_INVALID_ARG, fn, "projection needs N <= 128, nproj <= 4, proj and z");
  if (p->dropout_p < 0.f || p->dropout_p >= 1.f) return fail(GNN_ERR_INVALID_ARG, fn, "dropout p in [0,1)");
  if (p->dropout_p > 0.f && (int64_t)p->M * (int64_t)p->N >= ((int64_t)1 << 32))
    return fail(GNN_ERR_UNSUPPORTED, fn, "dropout element index (rows x width) must be < 2^32");
  if (bad_math(p->math)) return fail(GNN_ERR_INVALID_ARG, fn, "bad math mode");
  if (bad_dtype(p->a_dtype) || bad_dtype(p->c_dtype)) return fail(GNN_ERR_INVALID_ARG, fn, "bad dtype");
  if (p->M == 0) return GNN_OK;  // an empty call launches nothing and looks at nothing below
  if (p->mask && p->ldmask < p->N) return fail(GNN_ERR_INVALID_ARG, fn, "bad ldmask");
  if (const char* why = image_args_bad(p)) return fail(GNN_ERR_INVALID_ARG, fn, why);
  if (a.kmask && (!a.ap_h2 || !a.dropout || !aligned(a.kmask, 4)))
    return fail(GNN_ERR_INVALID_ARG, fn, "keep_mask needs a half-pair image A and dropout_p > 0");
  return GNN_OK;
}

enum NTKernel {  // NONE: an empty call launches nothing; IMG_*: A read from its image (gnn_gemm_nt_planes_ok)
  NT_NONE, NT_IMG_H2, NT_IMG_BF16, NT_IMG_SPLIT,
  NT_SKINNY_N, NT_SKINNY_K, NT_X3_BF16, NT_H2S, NT_X3, NT_F32_V4, NT_F32_V2, NT_F32_V1
};
struct NTPick { NTKernel kernel; gnn_status status; const char* why; };  // why != null: refused with status

// The kernel a validated NT call runs in `phase`, or why it is refused.
NTPick nt_select(const gnn_gemm_nt_params* p, const NTArgs& a, int phase) {
  auto run = [](NTKernel k) { return NTPick{k, GNN_OK, nullptr}; };
  auto no = [](gnn_status s, const char* why) { return NTPick{NT_NONE, s, why}; };
  auto ws = [&](size_t need) { return p->workspace && p->workspace_bytes >= need; };
  if (p->row_exp && (p->a_planes || p->colsum_part || phase != NT_PHASE_ALL))
    return no(GNN_ERR_UNSUPPORTED, "row_exp needs the in-kernel half-pair NT over f32 A1 / A2");
  if (a.M == 0 && phase != NT_PHASE_PREP) return run(NT_NONE);
  const NTSkinny skinny = nt_skinny_form(a);
  if (p->colsum_part) {  // ABI 21: the skinny-K form also writes C's per-block column sums
    if (skinny != SKINNY_K || p->a_planes || phase != NT_PHASE_ALL)
      return no(GNN_ERR_UNSUPPORTED, "colsum_part needs the skinny-K form (k1 <= 8, k2 = 0, 8 < N <= 256)");
    if (p->colsum_cap < (int64_t)nt_skinny_k_blocks(a) * p->N || !aligned(p->colsum_part, 4))
      return no(GNN_ERR_INVALID_ARG, "colsum_cap < gnn_gemm_nt_colsum_blocks x N");
    return run(NT_SKINNY_K);
  }
  const bool split = p->math != GNN_MATH_F32;
  if (p->a_planes) {  // the image kernels; a call that also gives f32 A1 / A2 falls back on those
    const bool img = split && !p->mask, planes_only = !p->a1;
    const size_t img_bytes = (size_t)(a.ap_ld / 16) * 3 * 256 * sizeof(uint4);
    if (a.ap_h2) {  // the half-pair image: f16 hi / lo planes, 3 products
      if (img && nt_h2_ok(a) && ws(img_bytes + BN * sizeof(float))) return run(NT_IMG_H2);
      if (planes_only) return no(GNN_ERR_UNSUPPORTED, "half-pair image A outside the half-pair kernel's shapes");
    }
    if (a.a_bf16) {  // a bf16 image (one plane): the bf16-storage form
      if (img && nt_img16_ok(a) && ws(img_bytes)) return run(NT_IMG_BF16);
      return no(GNN_ERR_UNSUPPORTED, "bf16 image A outside the image kernel's shapes");
    }
    if (img && nt_planes_ok(a) && ws(img_bytes)) return run(NT_IMG_SPLIT);
    if (planes_only) return no(GNN_ERR_UNSUPPORTED, "split-image A outside the planes kernel's shapes");
  }
  if (phase != NT_PHASE_ALL)  // prep_b / b_ready: only the image-A kernels have a separate B image
    return no(phase == NT_PHASE_PREP ? GNN_ERR_UNSUPPORTED : GNN_ERR_INVALID_ARG,
              "a separate B prep (prep_b / b_ready) needs an image-A kernel (gnn_gemm_nt_planes_ok)");
  const bool h2s = p->math == GNN_MATH_HALF_PAIR && nt_h2s_ok(a) && ws(nt_h2s_workspace(a.k1, a.k2));
  if (p->row_exp && !h2s)  // (checked before the skinny forms: a caller asking for row_exp gets it or an error)
    return no(GNN_ERR_UNSUPPORTED, "row_exp needs the in-kernel half-pair NT (GNN_MATH_HALF_PAIR, the w1/w2 "
                                   "form, N <= 128, k1 / k2 multiples of 16, k1 + k2 <= 128, f32, a workspace)");
  if (!p->row_exp && skinny != SKINNY_NONE)  // Nc <= 8 or K <= 8
    return run(skinny == SKINNY_N ? NT_SKINNY_N : NT_SKINNY_K);
  if (p->mask) return no(GNN_ERR_UNSUPPORTED, "the mask epilogue needs a skinny shape (K <= 8 or N <= 8)");
  if (a.a_bf16 || a.c_bf16) {
    if (!a.a_bf16 || !a.w1 || a.Nc > BN || !split)
      return no(GNN_ERR_UNSUPPORTED, "bf16 NT needs bf16 A, the w1/w2 form, N <= 128 and split math");
    return run(NT_X3_BF16);
  }
  if (h2s) return run(NT_H2S);                           // in-kernel half-pair (gemm_x3.hip, ABI 23)
  if (split && a.w1 && a.Nc <= BN) return run(NT_X3);  // split-bf16 MFMA (gemm_x3.hip)
  auto av = [&](int v) {
    return (a.k1 % v == 0) && (a.lda1 % v == 0) && aligned(a.a1, 4 * v) &&
           (a.k2 == 0 || ((a.k2 % v == 0) && (a.lda2 % v == 0) && aligned(a.a2, 4 * v)));
  };
  return run(av(4) ? NT_F32_V4 : av(2) ? NT_F32_V2 : NT_F32_V1);
}

// nt_select for a query that launches nothing: phase ALL of the call with a sufficient workspace
// (the queries have never looked at it) and, for the column-sum query, a column-sum buffer
NTPick nt_select_query(const gnn_gemm_nt_params* p, NTArgs* a, bool colsum) {
  gnn_gemm_nt_params q = *p;
  q.workspace = &q; q.workspace_bytes = SIZE_MAX; q.b_ready = 0;
  if (colsum) { q.colsum_part = reinterpret_cast<float*>(&q); q.colsum_cap = INT64_MAX; }
  nt_args(&q, a, nullptr);
  return nt_select(&q, *a, NT_PHASE_ALL);
}

gnn_status gemm_nt_dispatch(const gnn_gemm_nt_params* p, gnn_stream_t stream, const char* fn, int phase) {
  NTArgs a;
  if (const gnn_status s = nt_args(p, &a, fn)) return s;
  if (phase == NT_PHASE_ALL && p->b_ready) phase = NT_PHASE_RUN;
  const NTPick k = nt_select(p, a, phase);
  if (k.why) return fail(k.status, fn, k.why);
  hipStream_t st = (hipStream_t)stream;
  uint4* img = static_cast<uint4*>(p->workspace);
  if (k.kernel > NT_IMG_SPLIT) a.ap = nullptr;  // the f32 operands serve
  switch (k.kernel) {
    case NT_NONE: return GNN_OK;
    case NT_IMG_H2: launch_nt_h2(a, img, st, phase); break;
    case NT_IMG_BF16: launch_nt_img16(a, img, st, phase); break;
    case NT_IMG_SPLIT: launch_nt_ws_planes(a, img, st, phase); break;
    case NT_SKINNY_N:
    case NT_SKINNY_K: launch_nt_skinny(a, st); break;
    case NT_X3_BF16:
    case NT_X3: launch_nt_x3(a, p->workspace, p->workspace_bytes, st); break;
    case NT_H2S: launch_nt_h2s(a, p->workspace, st); break;
    default: launch_nt_f32(a, k.kernel == NT_F32_V4 ? 4 : k.kernel == NT_F32_V2 ? 2 : 1, st); break;
  }
  return hip_check(hipGetLastError(), fn);
}

}  // namespace

extern "C" gnn_status gnn_gemm_nt_workspace_size(int64_t N, int64_t k1, int64_t k2, size_t* bytes) {
  if (!bytes || N < 1 || k1 < 1 || k2 < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "bad args");
  // the image-A kernels (a_planes) size their B image by the image's row width (<= 336 columns,
  // 21 k-steps), not by k1 + k2: a narrow input on a 176-wide image runs 11 k-steps
  *bytes = N <= BN ? std::max(nt_x3_workspace(k1, k2), (size_t)21 * 3 * 256 * 16 + BN * sizeof(float)) : 0;
  return GNN_OK;
}

extern "C" gnn_status gnn_gemm_nt_f32(const gnn_gemm_nt_params* p, gnn_stream_t stream) {
  return gemm_nt_dispatch(p, stream, __func__, NT_PHASE_ALL);
}
extern "C" gnn_status gnn_gemm_nt_prep_b(const gnn_gemm_nt_params* p, gnn_stream_t stream) {
  return gemm_nt_dispatch(p, stream, __func__, NT_PHASE_PREP);
}

extern "C" gnn_status gnn_gemm_nt_colsum_blocks(const gnn_gemm_nt_params* p, int32_t* nb) {
  if (!p || !nb) return fail(GNN_ERR_INVALID_ARG, __func__, "null");
  NTArgs a;
  *nb = nt_select_query(p, &a, true).kernel == NT_SKINNY_K ? nt_skinny_k_blocks(a) : 0;
  return GNN_OK;
}

// Whether a call would read A from its image (the caller then needs no f32 A).
extern "C" int gnn_gemm_nt_planes_ok(const gnn_gemm_nt_params* p) {
  if (!p || !p->a_planes) return 0;
  NTArgs a;
  const NTKernel k = nt_select_query(p, &a, false).kernel;
  return k >= NT_IMG_H2 && k <= NT_IMG_SPLIT;
}

namespace gnnmp {
gnn_status nt_h2_prep_from_params(const gnn_gemm_nt_params* p, H2Prep* out, const char* fn) {
  NTArgs a;
  if (const gnn_status s = nt_args(p, &a, fn)) return s;
  if (nt_select(p, a, NT_PHASE_PREP).kernel != NT_IMG_H2 || !aligned(p->workspace, 16))
    return fail(GNN_ERR_UNSUPPORTED, fn, "prep_b needs NT params that select the half-pair NT (and its workspace)");
  *out = h2_prep_of(a, static_cast<uint4*>(p->workspace));
  return GNN_OK;
}
}  // namespace gnnmp

// ------------------------------------------------------------------------------------ TN

namespace {

// Row blocks of a TN launch over M rows on at most `cap` blocks: whole 32-row chunks, as few per
// block as cap blocks need, and no more blocks than that takes — every block has rows, so no block
// writes an all-zero slab for the reduce to read back (a strong-scaling shard: 213 instead of 256
// slabs at 27,196 rows, -17 % of the slab traffic).  (ceil(chunks / blocks) is `per` again:
// blocks <= cap gives (per - 1) · blocks <= (per - 1) · cap < chunks.)
struct TNRows { int blocks; int64_t rows; };
TNRows tn_rows(int64_t M, int cap) {
  const int64_t chunks = ceil_div(M, 32);
  if (chunks <= 0) return {1, 0};
  const int64_t per = ceil_div(chunks, cap);
  return {(int)ceil_div(chunks, per), per * 32};
}
// cap: one block per CU; the in-kernel half-pair TN at Nr <= 64, k1 + k2 <= 128 holds three blocks
// per CU (its LDS is sized by its k-tiles and 64 G rows, 47 KB): three times the blocks, so three
// times the chunk loads in flight per CU (its chunk loop is latency-bound: one 16-row chunk in
// flight per block)
constexpr int kTnBlocks = 256, kTnBlocksNarrow = 768;
bool tn_narrow(int64_t Nr, int64_t Kc, int32_t nproj) { return Nr <= 64 && Kc <= 128 && !nproj; }

// the largest M whose half-pair dz-form TN runs split-K block pairs (GNNMP_TN_KSPLIT_MAXM, A/B)
int64_t tn_ksplit_max_m() {
  static const int64_t v = [] {
    const char* e = std::getenv("GNNMP_TN_KSPLIT_MAXM");
    return e ? std::atoll(e) : (int64_t)32768;  // the 8-way shard (27k rows): TN + reduce 32.1 -> 30.9 us; 4-way (52k): slower
  }();
  return v;
}
// the half-pair dz form's row blocks: split-K pairs over half as many row blocks at shard-sized M
TNRows tn_dz_rows(int64_t M) { return tn_rows(M, M <= tn_ksplit_max_m() ? kTnBlocks / 2 : kTnBlocks); }

// whether each of a block's 8 waves walks at most one 64-row group of its rows_per_block rows
bool tn_wave_per_group(int64_t rows_per_block) { return (rows_per_block + 63) / 64 + 1 <= 8; }
// (ABI 26) the CSC sum of u inside the half-pair dz-form TN at such a row block (shard-sized M:
// 8-way shard 0.0947 -> 0.0923 ms per step, profiles/r105_csc_ab.txt); GNNMP_TN_CSC_INKERNEL=0 / 1
// forces it off / on (A/B)
bool tn_csc_in_kernel(int64_t rows_per_block) {
  static const int v = [] {
    const char* e = std::getenv("GNNMP_TN_CSC_INKERNEL");
    return e ? std::atoi(e) : -1;
  }();
  if (rows_per_block > 1792) return false;  // the block's dz rows staged in LDS (gemm_planes.hip dzb)
  if (v >= 0) return v != 0;
  return tn_wave_per_group(rows_per_block);
}
// (ABI 28) whether the dz-form TN at M rows walks activity flags: its row block is larger than the
// in-kernel CSC fold takes (without the env override: a rule of M alone, so the caller's CSC sum,
// the call-side one and GNNMP_TN_CSC=0 all reach the same kernel)
bool tn_active_pays(int64_t M) { return M >= 16 && !tn_wave_per_group(tn_dz_rows(M).rows); }
int64_t tn_active_bytes(int64_t M) { return (ceil_div(M, GNN_ACTIVE_ROWS) + 15) / 16 * 16; }
// The flag-driven TN's form, read at every call (A/B inside one process):
// GNNMP_TN_ACTIVE_SPLIT=0 runs its first form — one block per row block, one chunk of loads in
// flight — instead of TN_ACT_SPLIT column blocks per row block with loads TN_ACT_RING chunks deep;
// GNNMP_TN_EMPTY_SKIP=0 has the row blocks without a flagged chunk write their zero slabs and the
// reduce read them.  Every combination gives the same bits.
bool env_off(const char* name) {
  const char* e = std::getenv(name);
  return e && e[0] == '0' && !e[1];
}
bool tn_active_split() { return !env_off("GNNMP_TN_ACTIVE_SPLIT"); }
bool tn_empty_skip() { return !env_off("GNNMP_TN_EMPTY_SKIP"); }

// floats of a TN output: dW[Nr][Kc] | db[Nr] | dW2[nproj][Nr] | dzsum[nproj]; a slab holds them padded
int64_t tn_out_floats(int64_t Nr, int64_t Kc, int32_t nproj) { return Nr * Kc + Nr + (int64_t)nproj * Nr + nproj; }
int64_t tn_slab_stride(int64_t n_out) { return (n_out + 63) / 64 * 64; }
unsigned red_blocks(int64_t n_out) { return (unsigned)ceil_div(ceil_div(n_out, 4), kRedOut); }

// The one translation of TN params (fn as nt_args); the slabs are the caller's workspace.
gnn_status tn_args(const gnn_gemm_tn_params* p, TNArgs* out, const char* fn) {
  TNArgs a{};
  a.M = p->M; a.Nr = (int32_t)p->Nr;
  a.g = p->g; a.ldg = p->ldg; a.dz = p->dz; a.lddz = p->lddz; a.proj = p->proj; a.nproj = p->dz ? p->nproj : 0;
  a.h = p->h; a.ldh = p->ldh; a.hscale = p->hscale;
  a.gout = p->gout; a.ldgout = p->ldgout;
  a.a1 = p->a1; a.lda1 = p->lda1; a.k1 = (int32_t)p->k1;
  a.a2 = p->a2; a.lda2 = p->lda2; a.k2 = (int32_t)p->k2;
  a.slab_stride = tn_slab_stride(tn_out_floats(p->Nr, p->k1 + p->k2, a.nproj));
  a.rows_per_block = tn_rows(p->M, kTnBlocks).rows;
  a.a_bf16 = p->a_dtype == GNN_DTYPE_BF16; a.h_bf16 = p->h_dtype == GNN_DTYPE_BF16; a.g_bf16 = p->g_dtype == GNN_DTYPE_BF16;
  image_args(p, &a);
  // (ABI 25) the plain g form's block scale from the producer's row-group maxima (row blocks are
  // whole 32-row chunks, so every block covers whole GNN_ROWMAX_ROWS groups)
  a.growmax = (a.ap_h2 && !a.dz && a.g) ? p->g_rowmax : nullptr;
  a.rowexp = p->row_exp;
  if (const gnn_graph* cg = p->dz_graph) {  // (ABI 26) the folded CSC sum (tn_plan checks it can be taken)
    a.cptr = cg->colptr; a.cnbr = cg->row; a.cu = p->dz_u; a.ldu = p->ldu; a.ccols = p->dz_cols;
  }
  *out = a;
  if (!fn) return GNN_OK;

  if (p->M < 0 || p->Nr < 1 || p->Nr > 128 || p->k1 < 1 || p->k2 < 0 || p->k1 + p->k2 > KMAX)
    return fail(GNN_ERR_UNSUPPORTED, fn, "needs 1 <= Nr <= 128 and k1 + k2 <= 384");
  const bool planes_only = p->a_planes && !p->a1;
  if (!planes_only && (!p->a1 || (p->k2 > 0 && !p->a2) || p->lda1 < p->k1 || (p->k2 > 0 && p->lda2 < p->k2)))
    return fail(GNN_ERR_INVALID_ARG, fn, "bad A operands");
  if (p->dz) {
    if (p->nproj < 1 || p->nproj > MAXPROJ || !p->proj || p->lddz < p->nproj)
      return fail(GNN_ERR_INVALID_ARG, fn, "dz form needs 1 <= nproj <= 4 and proj");
  } else if (!p->g || p->ldg < p->Nr) {
    return fail(GNN_ERR_INVALID_ARG, fn, "need g (or dz + proj)");
  }
  if (p->h && p->ldh < p->Nr) return fail(GNN_ERR_INVALID_ARG, fn, "bad ldh");
  if (bad_math(p->math)) return fail(GNN_ERR_INVALID_ARG, fn, "bad math mode");
  if (p->gout && p->ldgout < p->Nr) return fail(GNN_ERR_INVALID_ARG, fn, "bad ldgout");
  return GNN_OK;
}

// (the first three read A from its image: gnn_gemm_tn_planes_ok)
enum TNKernel { TN_IMG_H2, TN_IMG_BF16, TN_IMG_SPLIT, TN_SKINNY, TN_H2S, TN_X3, TN_F32 };
enum TNCsc { TN_CSC_READ, TN_CSC_IN_KERNEL, TN_CSC_CALL_SIDE };  // how dz's CSC columns are formed
enum TNFlags { TN_FLAGS_NONE, TN_FLAGS_CALLER, TN_FLAGS_WORKSPACE };
struct TNPlan {
  TNKernel kernel;
  int blocks, nred;        // the launch's grid; the slabs it writes
  int64_t rows_per_block;
  bool ksplit;             // split-K block pairs: blocks = 2 nred
  bool act_split;          // flags: TN_ACT_SPLIT column blocks per row block: blocks = TN_ACT_SPLIT nred
  bool empty;              // flags: unflagged row blocks write their slab's empty word only, the reduce skips them
  TNCsc csc;               // CALL_SIDE: gnn_aggregate_active_f32 first
  TNFlags flags;           // dz's activity flags; WORKSPACE: at flags_off, written by the call-side CSC sum
  size_t flags_off;
  gnn_status status; const char* why;  // why != null: refused with status
};

// The launch a validated TN call with M > 0 makes over a workspace of ws_bytes, or why it is refused.
TNPlan tn_plan(const gnn_gemm_tn_params* p, const TNArgs& a, size_t ws_bytes, const uint8_t* dz_active) {
  TNPlan pl{};
  auto run = [&](TNKernel k) { pl.kernel = k; return pl; };
  auto no = [&](gnn_status s, const char* why) { pl.status = s; pl.why = why; return pl; };
  auto rows = [&](TNRows r) { pl.blocks = pl.nred = r.blocks; pl.rows_per_block = r.rows; };
  const size_t slab_bytes = (size_t)a.slab_stride * sizeof(float);
  rows(tn_rows(a.M, kTnBlocks));
  const size_t slabs_end = (size_t)pl.blocks * slab_bytes;
  const gnn_graph* cg = p->dz_graph;
  if (cg && (!p->dz || !p->dz_u || !cg->colptr || !cg->row || cg->num_nodes != p->M || p->dz_cols < 1 ||
             p->dz_cols > 2 || p->dz_cols > p->nproj || p->ldu < p->dz_cols))
    return no(GNN_ERR_INVALID_ARG, "dz_graph needs the dz form, dz_u, 1 <= dz_cols <= 2 and num_nodes == M");
  if (bad_dtype(p->a_dtype) || bad_dtype(p->h_dtype) || bad_dtype(p->g_dtype)) return no(GNN_ERR_INVALID_ARG, "bad dtype");
  if (a.g_bf16 && !(a.ap && a.a_bf16))
    return no(GNN_ERR_UNSUPPORTED, "bf16 g / gout need the bf16-image TN (a bf16 a_planes)");
  if (a.h_bf16 && !a.a_bf16) return no(GNN_ERR_UNSUPPORTED, "bf16 h needs bf16 A");
  if (const char* why = image_args_bad(p)) return no(GNN_ERR_INVALID_ARG, why);
  const bool split = p->math != GNN_MATH_F32, planes_only = a.ap && !a.a1;
  if (a.ap_h2) {  // the half-pair image: f16 hi / lo planes, 3 products
    if (dz_active && !(tn_h2_ok(a) && a.dz && !a.gout && !a.cptr))
      return no(GNN_ERR_UNSUPPORTED, "dz_active outside the half-pair dz-form TN's shapes");
    if (split && tn_h2_ok(a)) {
      // a shard-sized M (the dz form): split-K block pairs over half as many row blocks (round 6).
      // The flag-driven kernel never splits K, but it runs the row blocks of the dense call at the
      // same M (nred of them, rows_per_block each), so its sums are the dense call's, bit for bit
      if (a.dz) rows(tn_dz_rows(a.M));
      // (ABI 26) rows of more than one 64-row group per wave: the folded CSC sum would run two
      // dependent gather rounds per wave ahead of the chunk loop (full configs[1] graph, 800 rows a
      // block: TN 87 -> 94 us, profiles/r105_csc_ab.txt) — the separate narrow launch instead
      pl.csc = !a.cptr ? TN_CSC_READ : tn_csc_in_kernel(pl.rows_per_block) ? TN_CSC_IN_KERNEL : TN_CSC_CALL_SIDE;
      // (ABI 28) the call-side CSC sum also writes dz's activity flags (past the slabs) where they
      // pay, and the TN walks them: the same kernel the caller's own flagged CSC sum reaches
      if (dz_active) {
        pl.flags = TN_FLAGS_CALLER;
      } else if (pl.csc == TN_CSC_CALL_SIDE && tn_active_pays(a.M)) {
        pl.flags = TN_FLAGS_WORKSPACE;
        pl.flags_off = slabs_end;
        if (ws_bytes < slabs_end + (size_t)tn_active_bytes(a.M) || !aligned(a.slab, 16))
          return no(GNN_ERR_WORKSPACE, "workspace too small for the activity flags (gnn_gemm_tn_workspace_size)");
      }
      if (pl.flags != TN_FLAGS_NONE && pl.rows_per_block / GNN_ACTIVE_ROWS > TN_ACT_CAP)  // the block's chunk list is a fixed array
        return no(GNN_ERR_UNSUPPORTED, "dz_active: row block beyond the chunk list's capacity");
      pl.ksplit = a.dz && a.M <= tn_ksplit_max_m() && pl.flags == TN_FLAGS_NONE;
      if (pl.ksplit) pl.blocks = 2 * pl.nred;
      if (pl.flags != TN_FLAGS_NONE) {
        pl.act_split = tn_active_split();
        if (pl.act_split) pl.blocks = TN_ACT_SPLIT * pl.nred;
        // the empty word is the slab's last pad word (no workspace beyond the slabs): a shape whose
        // outputs fill the stride has none and writes every slab
        pl.empty = tn_empty_skip() && a.slab_stride > tn_out_floats(a.Nr, a.k1 + a.k2, a.nproj);
      }
      return run(TN_IMG_H2);
    }
    if (planes_only) return no(GNN_ERR_UNSUPPORTED, "half-pair image A outside the half-pair kernel's shapes");
  }
  if (a.cptr)  // only the half-pair dz-form kernel forms dz's CSC columns itself
    return no(GNN_ERR_UNSUPPORTED, "dz_graph outside the half-pair dz-form TN (gnn_gemm_tn_planes_ok)");
  if (a.ap && !a.ap_h2) {
    if (a.a_bf16) {  // a bf16 image (one plane): the bf16-storage form
      if (!split || !tn_img16_ok(a)) return no(GNN_ERR_UNSUPPORTED, "bf16 image A outside the image kernel's shapes");
      return run(TN_IMG_BF16);
    }
    if (split && tn_planes_ok(a)) return run(TN_IMG_SPLIT);
    if (planes_only) return no(GNN_ERR_UNSUPPORTED, "split-image A outside the planes kernel's shapes");
  }
  if (tn_skinny_ok(a)) {  // Nr <= 8 plain g form: VALU stream (gemm_skinny.hip)
    pl.blocks = pl.nred = tn_skinny_blocks(a.M);
    if (ws_bytes < (size_t)pl.blocks * slab_bytes) return no(GNN_ERR_WORKSPACE, "workspace too small");
    return run(TN_SKINNY);
  }
  // the split kernels index rows with 32-bit element offsets (ldmax: the widest row pitch) and load whole 16-row chunks
  const int64_t ldmax = std::max({a.lda1, a.k2 > 0 ? a.lda2 : 0, a.h ? a.ldh : 0, a.g ? a.ldg : 0, a.dz ? a.lddz : 0});
  const bool off32 = (a.M + 32) * ldmax < ((int64_t)1 << 31);
  if (a.a_bf16 && (!split || !off32 || a.M < 16))
    return no(GNN_ERR_UNSUPPORTED, "bf16 TN needs split math, M >= 16 and M*ld < 2^31");
  if (p->math == GNN_MATH_HALF_PAIR && tn_h2s_ok(a) && off32) {  // in-kernel half-pair MFMA (gemm_x3.hip, ABI 23)
    const TNRows narrow = tn_rows(a.M, kTnBlocksNarrow);
    if (tn_narrow(a.Nr, a.k1 + a.k2, a.nproj) && ws_bytes >= (size_t)narrow.blocks * slab_bytes) rows(narrow);
    return run(TN_H2S);
  }
  if (split && off32 && a.M >= 16) return run(TN_X3);  // split-bf16 MFMA (gemm_x3.hip)
  return run(TN_F32);
}

gnn_status gemm_tn_dispatch(const gnn_gemm_tn_params* p, float* out, void* workspace, size_t workspace_bytes,
                            gnn_stream_t stream, const uint8_t* dz_active = nullptr) {
  const char* fn = dz_active ? "gnn_gemm_tn_active_f32" : "gnn_gemm_tn_f32";
  if (!p || !out) return fail(GNN_ERR_INVALID_ARG, fn, "null params/out");
  if (dz_active) {  // (ABI 28) the half-pair dz form with h, no gout, no dz_graph (tn_plan checks the image's shape)
    if (!p->dz || !p->h || p->gout || p->dz_graph || !p->a_planes || p->planes_format != GNN_PLANES_HALF_PAIR ||
        p->math == GNN_MATH_F32 || p->M < 16)
      return fail(GNN_ERR_UNSUPPORTED, fn, "dz_active needs the half-pair dz form with h, no gout, no dz_graph, M >= 16");
    if (!aligned(dz_active, 16)) return fail(GNN_ERR_INVALID_ARG, fn, "dz_active must be 16-byte aligned");
  }
  TNArgs a;
  if (const gnn_status s = tn_args(p, &a, fn)) return s;
  a.slab = static_cast<float*>(workspace);
  const int64_t n_out = tn_out_floats(a.Nr, a.k1 + a.k2, a.nproj);
  if (!workspace || workspace_bytes < (size_t)tn_rows(a.M, kTnBlocks).blocks * a.slab_stride * sizeof(float))
    return fail(GNN_ERR_WORKSPACE, fn, "workspace too small");
  if (p->sq_partial && (!p->sq_step || p->sq_cap < 2 * (int64_t)red_blocks(n_out) + 1 || p->sq_skip_lo > p->sq_skip_hi))
    return fail(GNN_ERR_INVALID_ARG, fn, "sq_partial needs sq_step, sq_cap >= 2 nb + 1, skip_lo <= skip_hi");
  hipStream_t st = (hipStream_t)stream;
  if (p->M == 0) {
    if (!p->sq_partial) return hip_check(hipMemsetAsync(out, 0, n_out * sizeof(float), st), fn);
    launch_slab_reduce(a.slab, a.slab_stride, 0, out, n_out, p, st);
    return hip_check(hipGetLastError(), fn);  // zero slabs: out = 0, partials 0, the step snapshot
  }
  const TNPlan pl = tn_plan(p, a, workspace_bytes, dz_active);
  if (pl.why) return fail(pl.status, fn, pl.why);
  uint8_t* ws_flags = pl.flags == TN_FLAGS_WORKSPACE ? static_cast<uint8_t*>(workspace) + pl.flags_off : nullptr;
  if (pl.csc == TN_CSC_CALL_SIDE) {
    gnn_agg_params ag{};
    ag.mode = GNN_AGG_SUM; ag.transpose = 1;
    gnn_agg_active act{ws_flags, p->dz + p->dz_cols, p->lddz, a.nproj - p->dz_cols};  // flags: dz's other columns count
    const gnn_status s = gnn_aggregate_active_f32(p->dz_graph, &ag, p->dz_u, p->ldu, p->dz_cols,
                                                  const_cast<float*>(p->dz), p->lddz, &act, stream);
    if (s != GNN_OK) return s;
    a.cptr = nullptr;
  }
  a.rows_per_block = pl.rows_per_block;
  a.dz_active = pl.flags == TN_FLAGS_CALLER ? dz_active : ws_flags;
  a.slab_empty = pl.empty;
  if (pl.kernel >= TN_SKINNY) a.ap = nullptr;      // the f32 operands serve ...
  if (pl.kernel <= TN_SKINNY) a.rowexp = nullptr;  // ... and only the MFMA kernels over them read their row exponents
  switch (pl.kernel) {
    case TN_IMG_H2: launch_tn_h2(a, pl.blocks, st, pl.ksplit, pl.act_split); break;
    case TN_IMG_BF16: launch_tn_img16(a, pl.blocks, st); break;
    case TN_IMG_SPLIT: launch_tn_planes(a, pl.blocks, st); break;
    case TN_SKINNY: launch_tn_skinny(a, pl.blocks, st); break;
    case TN_H2S: launch_tn_h2s(a, pl.blocks, st); break;
    case TN_X3: launch_tn_x3(a, pl.blocks, st); break;
    case TN_F32: launch_tn_f32(a, pl.blocks, st); break;
  }
  if (const gnn_status s = hip_check(hipGetLastError(), fn)) return s;
  launch_slab_reduce(a.slab, a.slab_stride, pl.nred, out, n_out, p, st, pl.empty);
  return hip_check(hipGetLastError(), fn);
}

}  // namespace

extern "C" gnn_status gnn_gemm_tn_workspace_size(int64_t M, int64_t Nr, int64_t Kc, int32_t nproj, size_t* bytes) {
  if (!bytes || M < 0 || Nr < 1 || Kc < 1 || nproj < 0) return fail(GNN_ERR_INVALID_ARG, __func__, "bad args");
  int64_t nb = tn_rows(M, kTnBlocks).blocks;  // the most slabs any kernel tn_plan could name at this shape writes
  if (Nr <= 8 && nproj == 0) nb = std::max<int64_t>(nb, tn_skinny_blocks(M));  // TN_SKINNY (tn_skinny_ok)
  if (tn_narrow(Nr, Kc, nproj)) nb = std::max<int64_t>(nb, tn_rows(M, kTnBlocksNarrow).blocks);  // TN_H2S
  *bytes = (size_t)nb * tn_slab_stride(tn_out_floats(Nr, Kc, nproj)) * sizeof(float);
  // (ABI 28) TN_FLAGS_WORKSPACE: the dz form's activity flags, past the slabs of its kTnBlocks blocks
  if (nproj > 0 && tn_active_pays(M)) *bytes += (size_t)tn_active_bytes(M);
  return GNN_OK;
}

extern "C" int gnn_gemm_tn_active_pays(int64_t M) { return tn_active_pays(M) ? 1 : 0; }
extern "C" int gnn_gemm_tn_active_split(void) { return TN_ACT_SPLIT; }
extern "C" int gnn_gemm_tn_active_ring(void) { return TN_ACT_RING; }
extern "C" gnn_status gnn_gemm_tn_sq_blocks(int64_t n_out, int32_t* nb) {
  if (!nb || n_out < 1) return fail(GNN_ERR_INVALID_ARG, __func__, "bad args");
  *nb = (int32_t)red_blocks(n_out);
  return GNN_OK;
}

extern "C" gnn_status gnn_gemm_tn_f32(const gnn_gemm_tn_params* p, float* out, void* workspace,
                                      size_t workspace_bytes, gnn_stream_t stream) {
  return gemm_tn_dispatch(p, out, workspace, workspace_bytes, stream);
}
extern "C" gnn_status gnn_gemm_tn_active_f32(const gnn_gemm_tn_params* p, const uint8_t* dz_active, float* out,
                                             void* workspace, size_t workspace_bytes, gnn_stream_t stream) {
  return gemm_tn_dispatch(p, out, workspace, workspace_bytes, stream, dz_active);
}

// Whether a call would read A from its image; with dz_graph, 0 when it would launch the CSC sum first (the caller can as well).
extern "C" int gnn_gemm_tn_planes_ok(const gnn_gemm_tn_params* p) {
  if (!p || !p->a_planes || p->M < 1 || p->Nr < 1 || p->Nr > 128) return 0;
  TNArgs a;
  tn_args(p, &a, nullptr);
  const TNPlan pl = tn_plan(p, a, SIZE_MAX, nullptr);
  return !pl.why && pl.kernel <= TN_IMG_SPLIT && pl.csc != TN_CSC_CALL_SIDE;
}
