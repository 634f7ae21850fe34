/*
 * gnnmp.h — C ABI of the MI355X (gfx950) GNN message-passing library `libgnnmp.so`.
 *
 * This is the drop-in boundary for the one hot path of elliptic-gnn-project:
 * the neighbour aggregation that `torch_geometric.nn.{SAGEConv,GCNConv,GATConv}`
 * perform inside `src/models/gnn.py` (imported at gnn.py:8, called at
 * gnn.py:28,31,49,52,72,75,187,193).  PyG 2.5.3 (the CI pin,
 * .github/workflows/ci.yml:17,39) is not vendored in the reference; every entry
 * point below names the PyG operation it replaces.
 *
 * Conventions
 *  - All buffers are device pointers owned by the caller.  The library never
 *    allocates or frees device memory; scratch comes from a caller-provided
 *    workspace whose size is queried first.
 *  - Feature matrices are row-major [rows, F] with a leading dimension `ld`
 *    (elements).  Outputs are fully overwritten (no zero-init contract).
 *  - Graph arrays are int32 (N, E < 2^31).  `edge_index` is PyG's [2, E] int64
 *    layout: row 0 = source j, row 1 = target i (flow source_to_target).
 *  - Every launch goes on the caller's stream; no entry point synchronises the
 *    host except gnn_graph_build's optional stats read (documented there).
 *  - Errors: a gnn_status is returned; gnn_last_error() gives a thread-local
 *    message.  Reductions are atomic-free: results are bitwise reproducible.
 */
#ifndef GNNMP_H_
#define GNNMP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNMP_ABI_VERSION 32

typedef struct ihipStream_t* gnn_stream_t; /* == hipStream_t */

typedef enum {
  GNN_OK = 0,
  GNN_ERR_INVALID_ARG = 1,
  GNN_ERR_INDEX_OUT_OF_RANGE = 2, /* PyG: IndexError from index_select */
  GNN_ERR_HIP = 3,
  GNN_ERR_WORKSPACE = 4,
  GNN_ERR_UNSUPPORTED = 5
} gnn_status;

/* Self-loop handling applied while building a graph plan. */
typedef enum {
  GNN_LOOPS_KEEP = 0,    /* SAGEConv: edges used exactly as given (duplicates and loops kept) */
  GNN_LOOPS_REPLACE = 1  /* GCNConv add_remaining_self_loops / GATConv remove_self_loops +
                            add_self_loops: drop every existing loop, then one loop per node,
                            placed LAST in its CSR row and CSC column (PyG appends loops). */
} gnn_loop_mode;

/*
 * A graph plan: CSR by destination (aggregation, forward) and CSC by source
 * (transpose, backward), both stable in PyG edge order.
 */
/*
 * Long-segment split of one plan direction (see gnn_split_build).  Aggregations over a
 * split direction run the truncated segments in the main pass, reduce the remaining pieces
 * of long segments into a caller-provided partial buffer, and combine them in piece order.
 */
typedef struct {
  int32_t seg_len;            /* T: slots per piece */
  int32_t reserved;
  int64_t num_long;           /* segments with more than T slots */
  int64_t num_pieces;         /* pieces of the long segments (ceil(deg / T) each) */
  const int32_t* ptr;         /* [N+1] segment pointer, every segment truncated to <= T slots */
  const int32_t* nbr;         /* truncated segments' neighbours (PyG order kept) */
  const int32_t* piece0;      /* [N] partial-sum row of piece 0 of a long segment, -1 if short */
  const int32_t* piece_seg;   /* [num_pieces] segment of each piece */
  const int32_t* long_seg;    /* [num_long] the long segments */
  const int32_t* order;       /* optional [N]: ptr/nbr position i holds segment order[i] (degree
                                 order, longest first, stable); NULL: position i = segment i */
} gnn_split;

typedef struct {
  int64_t num_nodes;
  int64_t num_slots;        /* stored edges (after loop handling) */
  const int32_t* rowptr;    /* [N+1] CSR by target i */
  const int32_t* col;       /* [S]   source j of each CSR slot */
  const int32_t* colptr;    /* [N+1] CSC by source j */
  const int32_t* row;       /* [S]   target i of each CSC slot */
  const int32_t* csc2csr;   /* [S]   CSR slot holding the same edge as each CSC slot */
  const gnn_split* csr_split; /* optional (NULL): long-row split of the CSR direction */
  const gnn_split* csc_split; /* optional (NULL): long-column split of the CSC direction */
} gnn_graph;

int gnn_abi_version(void);
const char* gnn_status_string(gnn_status s);
const char* gnn_last_error(void);

/* ------------------------------------------------------------------------ */
/* K0  graph plan build  (replaces the implicit per-call index handling of
 *     MessagePassing.propagate, and remove/add_(remaining_)self_loops)      */
/* ------------------------------------------------------------------------ */
gnn_status gnn_graph_workspace_size(int64_t num_nodes, int64_t num_edges, size_t* bytes);

/*
 * Build a plan from edge_index [2,E] int64 (contiguous).  Output arrays must
 * hold S_max = E (KEEP) or E + N (REPLACE) slots; rowptr/colptr N+1.
 * csr_eid[s] = PyG edge id of CSR slot s (original id; loop of node i = E + i).
 * stats (device int32[4], zeroed by this call): {S, n_input_loops, n_bad_index, 0}.
 * A non-zero n_bad_index means some index was outside [0, N): the plan is invalid
 * (PyG raises IndexError); the caller reads stats after the stream completes.
 */
gnn_status gnn_graph_build(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes,
                           gnn_loop_mode loops, int32_t* rowptr, int32_t* col, int32_t* csr_eid,
                           int32_t* colptr, int32_t* row, int32_t* csc2csr, int32_t* stats,
                           void* workspace, size_t workspace_bytes, gnn_stream_t stream);

/*
 * K0b  long-segment split of one direction (ptr/nbr = rowptr/col or colptr/row).
 * gnn_split_count writes {S_trunc, num_long, num_pieces} to device int64 counts[3] (the
 * caller reads them after the stream completes and sizes the outputs: tptr N+1, tnbr S_trunc,
 * piece0 N, piece_seg num_pieces, long_seg num_long).  gnn_split_build fills them; with
 * order (N entries, optional) the truncated tptr/tnbr are laid out in degree order (see
 * gnn_split.order) — the lane-group gather (8 < F <= 32·vec) runs its main pass in that order.
 */
gnn_status gnn_split_workspace_size(int64_t num_segs, size_t* bytes);
gnn_status gnn_split_count(const int32_t* ptr, int64_t num_segs, int32_t seg_len, int64_t* counts,
                           gnn_stream_t stream);
gnn_status gnn_split_build(const int32_t* ptr, const int32_t* nbr, int64_t num_segs, int32_t seg_len,
                           int32_t* tptr, int32_t* tnbr, int32_t* piece0, int32_t* piece_seg,
                           int32_t* long_seg, int32_t* order, void* workspace, size_t workspace_bytes,
                           gnn_stream_t stream);

/* deg[i] = number of CSR slots of i as float (PyG `count` / `deg`, gnn.py:49 via SAGEConv mean). */
gnn_status gnn_in_degree_f32(const gnn_graph* g, float* deg, gnn_stream_t stream);

/* K3  gcn_norm (PyG torch_geometric.nn.conv.gcn_conv.gcn_norm, improved=False, add_self_loops=True):
 *     dinv[i] = deg_i^-1/2 (inf -> 0) on a GNN_LOOPS_REPLACE plan.  Edge weight of (j -> i) is
 *     dinv[j]*dinv[i], formed inside the aggregation kernels.  Replaces GCNConv.forward's norm. */
gnn_status gnn_gcn_norm_f32(const gnn_graph* g, float* dinv, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K1/K2/K4  segmented aggregation over a plan (atomic-free)                */
/* ------------------------------------------------------------------------ */
typedef enum {
  GNN_AGG_SUM = 0,       /* y_r = sum_k x[nbr_k]                                          */
  GNN_AGG_MEAN = 1,      /* y_r = (sum_k x[nbr_k]) / max(nodew[r],1)  — SAGEConv aggr='mean' fwd (K1) */
  GNN_AGG_MEAN_BWD = 2,  /* y_r = sum_k x[nbr_k] / max(nodew[nbr_k],1) — mean backward over CSC (K2)  */
  GNN_AGG_GCN = 3,       /* y_r = sum_k (nodew[nbr_k]*nodew[r]) * x[nbr_k] — GCNConv propagate (K4)    */
  GNN_AGG_EDGE_W = 4     /* y_r = sum_k ew[slot_k, head(f)] * x[nbr_k, f] — GAT alpha-weighted (K5/K6) */
} gnn_agg_mode;

typedef struct {
  gnn_agg_mode mode;
  int32_t transpose;      /* 0: iterate CSR rows (targets gather sources); 1: CSC (sources gather targets) */
  const float* nodew;     /* per-node weights (deg for MEAN*, dinv for GCN) */
  const float* ew;        /* EDGE_W: per-CSR-slot weights [S, heads] */
  int32_t heads;          /* EDGE_W: feature f uses head f / (F / heads) */
  const float* addend;    /* optional [rows, F] added after the aggregation (ld_add) */
  int64_t ld_add;
  const float* bias;      /* optional [F] */
  int32_t relu;           /* apply max(.,0) last */
  float* part;            /* partial sums for a split direction: >= num_pieces * F floats; NULL or
                             too small -> the direction is aggregated unsplit */
  size_t part_bytes;
  float dropout_p;        /* > 0: F.dropout after bias / ReLU, element r*F + f kept by the counter
                             hash of gnn_gemm_nt_params (oracle/dropout_hash.py), kept values
                             scaled by 1/(1-p) — GCNNet's hidden layers (src/models/gnn.py:29-30) */
  uint64_t seed;
  const int64_t* seed_ptr; /* optional device counter: seed = *seed_ptr * 0x9E3779B97F4A7C15 + seed */
  const float* addend2;   /* optional (ABI 20, f32 only): a second [rows, F] term added after addend
                             (ld_add2) — a residual branch's gradient summed in the same store
                             (SAGE-ResBN's identity residual: dx = meanᵀ(dG_l) + dG_r + dr) */
  int64_t ld_add2;
} gnn_agg_params;

/* Generic fp32 aggregation: y[r, 0:F] for r in [0, N). */
gnn_status gnn_aggregate_f32(const gnn_graph* g, const gnn_agg_params* p, const float* x,
                             int64_t ldx, int64_t F, float* y, int64_t ldy, gnn_stream_t stream);

/* Row-group granularity of the activity flags (ABI 28). */
#define GNN_ACTIVE_ROWS 16

/* (ABI 28) Activity flags of an aggregation's output, written by the launch that finishes it: one
 * byte per group of GNN_ACTIVE_ROWS rows, row_active[r / 16] != 0 iff some row of the group has a
 * nonzero value (v != 0.0f, so NaN counts) among its F outputs or among active_with[r, 0:cols] —
 * the other columns of the buffer y is a slice of (the SAGE backward's dz = [Σ_CSC u | dlogits]:
 * y the left half, active_with the right).  A superset is legal, a 0 on a nonzero group never: a
 * group holding a row that a later pass of the call finishes is flagged 1.  The weight-gradient TN
 * reads them as its dz_active (gnn_gemm_tn_active_f32).  row_active: [ceil(N / 16)] bytes, 4-byte
 * aligned; active_with optional (cols 0..4, ld_active_with >= cols). */
typedef struct {
  uint8_t* row_active;
  const float* active_with;
  int64_t ld_active_with;
  int32_t active_with_cols;
} gnn_agg_active;

/* gnn_aggregate_f32 that also writes `act` (NULL or act->row_active NULL: exactly gnn_aggregate_f32).
 * Only the narrow slot-parallel form takes it (F <= 4; F <= 2 for GCN; not EDGE_W): every other
 * form is refused with GNN_ERR_UNSUPPORTED before any launch. */
gnn_status gnn_aggregate_active_f32(const gnn_graph* g, const gnn_agg_params* p, const float* x, int64_t ldx,
                                    int64_t F, float* y, int64_t ldy, const gnn_agg_active* act,
                                    gnn_stream_t stream);

/* bf16-storage form: x and y hold bf16 ([rows, F], ld in elements), f32 accumulation in plan
 * order, y rounded once (RNE).  Modes SUM / MEAN / MEAN_BWD / GCN (no EDGE_W); addend f32. */
gnn_status gnn_aggregate_bf16(const gnn_graph* g, const gnn_agg_params* p, const void* x, int64_t ldx,
                              int64_t F, void* y, int64_t ldy, gnn_stream_t stream);

/* Split images ("planes"): an f32 matrix held as three bf16 planes hi / mid / lo with
 * v = hi + mid + lo exactly (hi = RNE(v), mid = RNE(v - hi), lo = RNE(v - hi - mid)); plane p
 * at img + p*plane_stride elements, element (r, c) at r*ld + c.  The split-bf16 GEMMs read them
 * instead of splitting f32 operands in-kernel (gnn_gemm_nt_params / gnn_gemm_tn_params .a_planes).
 *
 * gnn_split_planes_f32: columns [col0, col0 + width) of rows [0, rows) <- planes of x [rows, F]
 * (zeros at columns >= F; width, col0, ld, plane_stride even). */
gnn_status gnn_split_planes_f32(const float* x, int64_t ldx, int64_t rows, int64_t F, void* img, int64_t ld,
                                int64_t plane_stride, int64_t col0, int64_t width, gnn_stream_t stream);
/* K1 with a split-image store: columns [0, width) of img <- planes of mean_{j->i} x[j]
 * (SAGEConv aggr='mean', the same arithmetic as gnn_sage_mean_fwd_f32), zeros at columns >= F.
 * Wide rows only (even F, 32 < F / vec with vec = 4 or 2, width / vec <= 128): UNSUPPORTED otherwise. */
gnn_status gnn_sage_mean_fwd_planes(const gnn_graph* g, const float* deg, const float* x, int64_t ldx, int64_t F,
                                    void* img, int64_t ld, int64_t plane_stride, int64_t width,
                                    gnn_stream_t stream);

/* Half-pair images: an f32 matrix held as TWO f16 planes of its PRE-SCALED values
 * u = v * 2^scale_exp:  hi = RNE_f16(u), lo = RNE_f16((u - hi) * 2^11), so u = hi + 2^-11 lo to
 * 2^-22 |u| while hi and (u - hi) * 2^11 are f16 normals, i.e. |u| >= 2^-13 (below that the pair
 * holds u to an absolute 2^-36).  The caller picks scale_exp per matrix so that its largest
 * magnitude lands in [2^13, 2^14): scale_exp = 14 - E with max|v| in [2^(E-1), 2^E) (0 for an
 * all-zero matrix; |scale_exp| <= 100).  Every value within 2^-26 of the matrix's largest then
 * keeps the full 2^-22 relative precision, whatever the matrix's overall magnitude (ABI 19: the
 * unscaled images of ABI 18 lost it below |v| ~ 2^-13).  |u| must stay below 2^15 (f16 range with
 * headroom for the agg half, a mean of the x rows).  The consuming GEMMs undo the scale exactly
 * (gnn_gemm_nt_params / gnn_gemm_tn_params .planes_exp, a power of two in their epilogues).  The
 * half-pair GEMMs (planes_format = GNN_PLANES_HALF_PAIR) run 3 f16 products per product instead
 * of the split-bf16 form's 6 and move 4 B per element instead of 6.  Otherwise the same layout and
 * arguments as the split-bf16 functions above. */
gnn_status gnn_split_h2_f32(const float* x, int64_t ldx, int64_t rows, int64_t F, void* img, int64_t ld,
                            int64_t plane_stride, int64_t col0, int64_t width, int32_t scale_exp,
                            gnn_stream_t stream);
/* gnn_sage_mean_fwd_h2: K1 with a half-pair store of mean_{j->i} x[j] * 2^scale_exp (the mean
 * rounded as gnn_sage_mean_fwd_f32 rounds it, then scaled exactly; scale_exp = the exponent of
 * the image's x half, so |agg * 2^scale_exp| <= max|x * 2^scale_exp|).  It optionally also writes
 * the dropout keep bits of the NT that consumes the
 * image (keep_mask != NULL, [num_nodes][4] uint32, 16-byte aligned; the NT reads the words of
 * ceil(num_nodes / 32) * 32 rows, clamping the row index into [0, num_nodes)): bit c of
 * keep_mask[r*4 + c/32] = keep_elem(seed', r*mask_cols + c) with seed' the NT's (seed, seed_ptr)
 * rule — the mask the NT would hash itself, computed where the gather leaves the VALU idle
 * (gnn_gemm_nt_params.keep_mask).
 * prep_b (optional): the params of the half-pair NT that reads this image (a_planes == img and
 * planes_exp == scale_exp); its B-image prep (gnn_gemm_nt_prep_b) runs inside this launch, on
 * extra blocks beside the gather, for a later gnn_gemm_nt_f32 of the same params with
 * b_ready = 1.  UNSUPPORTED when the params do not select the half-pair NT.
 * hub (optional, ABI 21; NULL or num_long == 0: one wave per 16 rows throughout): the rows r with
 * deg[r] > hub->seg_len (hub->long_seg, num_long of them) are each walked by a block of their own
 * (4 waves over interleaved 8-slot groups, summed in wave order) instead of by the wave holding
 * them; hub->ptr / nbr are the CSR with those rows' slots removed (natural order: order and
 * piece0 NULL; num_pieces, piece_seg unused).  For small graphs (a strong-scaling shard), where
 * the one wave walking a hub row is the launch's tail.  Changes the hub rows' summation order
 * (within the mean's rounding), not the other rows'.  hub->piece_seg (optional): [num_pieces + 1]
 * non-decreasing row boundaries from 0 to num_nodes, wave k of the main pass taking rows
 * [piece_seg[k], piece_seg[k + 1]) (at most 64; balanced by slots instead of 16 rows each). */
struct gnn_gemm_nt_params;
gnn_status gnn_sage_mean_fwd_h2(const gnn_graph* g, const float* deg, const float* x, int64_t ldx, int64_t F,
                                void* img, int64_t ld, int64_t plane_stride, int64_t width, int32_t scale_exp,
                                uint32_t* keep_mask, int64_t mask_cols, float dropout_p, uint64_t seed,
                                const uint64_t* seed_ptr, const struct gnn_gemm_nt_params* prep_b,
                                const gnn_split* hub, gnn_stream_t stream);
typedef enum {
  GNN_PLANES_SPLIT_BF16 = 0,  /* 3 bf16 planes hi / mid / lo (gnn_split_planes_f32) */
  GNN_PLANES_HALF_PAIR = 1    /* 2 f16 planes hi / lo (gnn_split_h2_f32) */
} gnn_planes_format;

/* The SAGE output layer's mean and the training loss in ONE pass (ABI 19): logits = mean_{j->i}
 * z[j, 0:C] + z[i, C:2C] + bias (SAGEConv transform-first: z = h·[W_l ; W_r]ᵀ, gnn.py:49-53) —
 * gnn_aggregate_f32(MEAN, addend, bias)'s arithmetic — and, in the same kernel's epilogue, the
 * masked class-weighted cross entropy of those logits (gnn_masked_ce_f32: dlogits, per-256-row loss
 * partials in `workspace`, `loss` = Σ partials · inv_denom or left to gnn_masked_ce_finish /
 * gnn_adam_group.loss_partial when NULL), bit for bit as the two calls produce them.  Replaces
 * the F = 2 aggregation + the CE launch of the training step (src/train_gnn.py:192-199).
 * 1 <= C <= 4, ldz >= 2C; workspace: gnn_masked_ce_workspace_size(num_nodes).  u (optional, ABI 20,
 * [N, C], ldu >= C): dlogits / max(deg, 1) per row — the transposed mean's per-slot term, so the
 * backward's meanᵀ(dlogits) is a plain CSC sum of u (gnn_aggregate_f32 SUM, transpose), bit for bit
 * the MEAN_BWD result, without the per-slot degree gather and division.  colsum (optional, ABI 21):
 * dlogits' per-256-row-block column sums as gnn_masked_ce_colsum_f32 writes them (the output
 * bias gradient through gnn_colsum_finish_f32: SAGE-ResBN's output conv). */
gnn_status gnn_sage_out_mean_ce_f32(const gnn_graph* g, const float* deg, const float* z, int64_t ldz, int32_t C,
                                    const float* bias, float* logits, int64_t ldo, const int64_t* y,
                                    const uint8_t* mask, const float* class_w, float inv_denom, float* dlogits,
                                    int64_t ld_d, float* u, int64_t ldu, float* colsum, float* loss, void* workspace,
                                    size_t workspace_bytes, gnn_stream_t stream);

/* Named forms of the above (what an FFI binding of SAGEConv would call). */
gnn_status gnn_sage_mean_fwd_f32(const gnn_graph* g, const float* deg, const float* x, int64_t ldx,
                                 int64_t F, float* out, int64_t ldo, gnn_stream_t stream);
gnn_status gnn_sage_mean_bwd_f32(const gnn_graph* g, const float* deg, const float* dout,
                                 int64_t ld_dout, int64_t F, float* dx, int64_t ld_dx,
                                 gnn_stream_t stream);

/* Explain mode (PyG MessagePassing.propagate with `explain` on: every message multiplied by
 * edge_mask[e] before aggregation; driven by GNNExplainer, src/analysis/explain.py:593-672).
 * Forward and x-gradient run as GNN_AGG_EDGE_W with the mask as slot weight; this entry point
 * gives the mask gradient: out[eid ? eid[s] : s] = <a[r], b[col[s]]> / max(nodew[r], 1)
 * (nodew NULL: / 1) for every CSR slot s of row r — for SAGEConv's mean a = dOut, b = x. */
gnn_status gnn_edge_dot_f32(const gnn_graph* g, const int32_t* eid, const float* nodew, const float* a,
                            int64_t lda, const float* b, int64_t ldb, int64_t F, float* out,
                            gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K5/K6  GATConv edge softmax + aggregation (PyG GATConv.edge_update/message, utils.softmax) */
/* ------------------------------------------------------------------------ */
/* a_src[n,h] = <xh[n,h,:], att_src[h,:]>, a_dst likewise. xh is [N, H*C] (ld_xh). */
gnn_status gnn_gat_scores_f32(int64_t N, int32_t H, int32_t C, const float* xh, int64_t ld_xh,
                              const float* att_src, const float* att_dst, float* a_src,
                              float* a_dst, gnn_stream_t stream);

/* Fused forward over a GNN_LOOPS_REPLACE plan: e = leaky_relu(a_src[j]+a_dst[i], slope);
 * alpha = exp(e - max_i) / (sum_i exp + 1e-16); out[i] = sum alpha * xh[j]
 * (concat: [N,H*C]; else head-mean [N,C]) + bias.  alpha saved per CSR slot [S,H]. */
gnn_status gnn_gat_fwd_f32(const gnn_graph* g, int32_t H, int32_t C, int32_t concat, float slope,
                           const float* xh, int64_t ld_xh, const float* a_src, const float* a_dst,
                           const float* bias, float* alpha, float* out, int64_t ldo,
                           gnn_stream_t stream);

/* Fused forward, scores in-kernel: a_src / a_dst are formed from the gathered xh rows and the
 * attention vectors (no gnn_gat_scores_f32 pass; both are written out for the backward), and
 * GATNet's hidden-layer activation is applied on the store (src/models/gnn.py:72-74):
 *   out = dropout(act(sum_j alpha_ij xh[j] + bias))   act = GNN_ACT_NONE | GNN_ACT_ELU (alpha 1)
 * dropout as in gnn_gemm_nt_params: keep iff hash(seed, row*F_out + col) < 1-p, kept / (1-p).
 * Same softmax as gnn_gat_fwd_f32 (one-pass online max / sum, merged in a fixed order). */
typedef enum { GNN_ACT_NONE = 0, GNN_ACT_ELU = 1 } gnn_act;
typedef struct {
  int32_t heads, chans, concat;
  float slope;
  const float* xh; int64_t ld_xh;         /* [N, H*C] */
  const float* att_src; const float* att_dst;  /* [H*C] */
  const float* bias;                      /* optional [F_out] */
  gnn_act act;
  float dropout_p;                        /* 0 = off */
  uint64_t seed; const uint64_t* seed_ptr; /* as gnn_gemm_nt_params */
  float* a_src; float* a_dst;             /* out [N, H] */
  float* alpha;                           /* out [S, H] */
  float* out; int64_t ldo;                /* out [N, F_out] */
  const float* edge_w;                    /* optional [S]: explain mode (PyG propagate with
                                             `_explain`): every message alpha * xh[j] of CSR slot s is
                                             multiplied by edge_w[s] after the softmax */
  const float* proj; int32_t nproj;       /* optional (ABI 24, concat layers): z = out · projᵀ written */
  float* z; int64_t ldz;                  /* beside the store, proj [nproj, H·C] (16-byte aligned,
                                             nproj <= 4) — GATNet's output conv's lin (gnn.py:75) on the
                                             hidden layer's stored rows, so its input is never read back */
} gnn_gat_fwd_params;
gnn_status gnn_gat_fwd_fused_f32(const gnn_graph* g, const gnn_gat_fwd_params* p, gnn_stream_t stream);
/* GATNet's output conv (src/models/gnn.py:67,75: heads 1, C <= 2, concat False, no act / dropout /
 * edge_w) in the narrow slot-parallel form, optionally with the masked CE in the same launch
 * (round 6, ABI 22): out, a_src, a_dst and alpha exactly as gnn_gat_fwd_fused_f32 defines them
 * (online softmax per row; fp32-close, not bitwise, to the lane-group kernel), then — y non-NULL —
 * gnn_masked_ce_f32 of the logits with its workspace contract (loss NULL: partials deferred),
 * dlogits, and colsum (optional) the per-256-row-block column sums of dlogits as
 * gnn_masked_ce_colsum_f32 writes them.  N >= 1. */
gnn_status gnn_gat_out_ce_f32(const gnn_graph* g, const gnn_gat_fwd_params* p, const int64_t* y, const uint8_t* mask,
                              const float* class_w, float inv_denom, float* dlogits, int64_t ld_d, float* colsum,
                              float* loss, void* workspace, size_t workspace_bytes, gnn_stream_t stream);

/* Gradient through y = dropout(act(pre)) from y itself (F.elu / F.dropout backward, gnn.py:73-74):
 * dpre = dy * keep * 1/(1-p) * act'(pre), ELU' = 1 for y > 0 else exp(pre) = y*(1-p) + 1.
 * [N, F]; dpre may alias dy. */
gnn_status gnn_gat_act_bwd_f32(int64_t N, int64_t F, gnn_act act, float dropout_p, uint64_t seed,
                               const uint64_t* seed_ptr, const float* y, int64_t ldy, const float* dy,
                               int64_t lddy, float* dpre, int64_t ld_dpre, gnn_stream_t stream);

/* Backward.  dout is [N,H*C] (concat) or [N,C].  Produces dxh [N,H*C] (includes the score
 * paths through att_src/att_dst), d_att_src/d_att_dst [H*C].  workspace from
 * gnn_gat_bwd_workspace_size. */
gnn_status gnn_gat_bwd_workspace_size(int64_t N, int64_t S, int32_t H, int32_t C, size_t* bytes);
gnn_status gnn_gat_bwd_f32(const gnn_graph* g, int32_t H, int32_t C, int32_t concat, float slope,
                           const float* xh, int64_t ld_xh, const float* a_src, const float* a_dst,
                           const float* att_src, const float* att_dst, const float* alpha,
                           const float* dout, int64_t ld_dout, float* dxh, int64_t ld_dxh,
                           float* d_att_src, float* d_att_dst, void* workspace,
                           size_t workspace_bytes, gnn_stream_t stream);

/* Backward of a hidden GATConv whose output went through dropout(act(.)) in the forward store
 * (gnn_gat_fwd_fused_f32 with act / dropout_p; concat heads): dy is the gradient of the stored
 * y; d pre = dy * keep / (1-p) * act'(pre) (gnn_gat_act_bwd_f32's formula) is formed inside the
 * rows pass as each row is loaded and written to dpre [N, H*C] (the cols pass and the bias
 * gradient read it); otherwise as gnn_gat_bwd_f32.  Replaces the act / dropout backward of
 * GATNet's hidden layers (src/models/gnn.py:73-74) fused with GATConv's. */
gnn_status gnn_gat_bwd_act_f32(const gnn_graph* g, int32_t H, int32_t C, float slope, const float* xh,
                               int64_t ld_xh, const float* a_src, const float* a_dst, const float* att_src,
                               const float* att_dst, const float* alpha, gnn_act act, float dropout_p,
                               uint64_t seed, const uint64_t* seed_ptr, const float* y, int64_t ld_y,
                               const float* dy, int64_t ld_dy, float* dpre, int64_t ld_dpre, float* dxh,
                               int64_t ld_dxh, float* d_att_src, float* d_att_dst, void* workspace,
                               size_t workspace_bytes, gnn_stream_t stream);

/* (ABI 24) gnn_gat_bwd_act_f32 with dy given as dz · proj (dz [N, nproj], ld_dz; proj [nproj, H·C],
 * 16-byte aligned, nproj <= 4): the backward of a hidden layer whose output fed a projection
 * (gnn_gat_fwd_params.proj) — dy is formed as each row slice loads, never stored.
 * (ABI 25) dxh_rowmax (optional, [ceil(N / GNN_ROWMAX_ROWS)] uint32): also the float bits of max |dxh|
 * over each group of GNN_ROWMAX_ROWS rows — the g_rowmax of the weight-gradient TN of the layer's
 * lin (dW = dxhᵀ · x), which then skips its own pass over dxh. */
gnn_status gnn_gat_bwd_act_proj_f32(const gnn_graph* g, int32_t H, int32_t C, float slope, const float* xh,
                                    int64_t ld_xh, const float* a_src, const float* a_dst, const float* att_src,
                                    const float* att_dst, const float* alpha, gnn_act act, float dropout_p,
                                    uint64_t seed, const uint64_t* seed_ptr, const float* y, int64_t ld_y,
                                    const float* dz, int64_t ld_dz, const float* proj, int32_t nproj, float* dpre,
                                    int64_t ld_dpre, float* dxh, int64_t ld_dxh, float* d_att_src, float* d_att_dst,
                                    uint32_t* dxh_rowmax, void* workspace, size_t workspace_bytes,
                                    gnn_stream_t stream);

/* Explain-mode backward (messages scaled by edge_w[s], see gnn_gat_fwd_params.edge_w): as
 * gnn_gat_bwd_f32, plus d_edge_w[s] = sum_h alpha[s,h] * <dout_i(h), xh[j,h,:]> for every CSR slot. */
gnn_status gnn_gat_bwd_ew_f32(const gnn_graph* g, int32_t H, int32_t C, int32_t concat, float slope,
                              const float* xh, int64_t ld_xh, const float* a_src, const float* a_dst,
                              const float* att_src, const float* att_dst, const float* alpha,
                              const float* dout, int64_t ld_dout, float* dxh, int64_t ld_dxh,
                              float* d_att_src, float* d_att_dst, const float* edge_w, float* d_edge_w,
                              void* workspace, size_t workspace_bytes, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K7  fp32 MFMA GEMMs with the surrounding elementwise work fused in.      */
/*     Replace PyG Linear lin_l/lin_r/lin (gnn.py:20-23,41-44,64-67) and the  */
/*     F.relu + F.dropout between layers (gnn.py:29-30,50-51,73-74).          */
/* ------------------------------------------------------------------------ */
/* Element type of a feature buffer. */
typedef enum { GNN_DTYPE_F32 = 0, GNN_DTYPE_BF16 = 1 } gnn_dtype;

/* Arithmetic of the K7 GEMMs.  Both are fp32-accurate (inputs, outputs and accumulation f32). */
typedef enum {
  GNN_MATH_SPLIT_BF16 = 0, /* default: every f32 operand split into hi+mid+lo bf16 terms, 6 products on
                              v_mfma_f32_32x32x16_bf16 (dropped terms <= ~2^-23 relative per product);
                              used for the w1/w2 NT form and the TN kernel, else falls back to: */
  GNN_MATH_F32 = 1,        /* exact f32 MFMA (v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain) */
  GNN_MATH_HALF_PAIR = 2   /* (ABI 23) f32 operands split in the kernel into half-pair f16 terms
                              (hi = RNE_f16(v·s), lo = RNE_f16((v·s − hi)·2^11)), 3 products on
                              v_mfma_f32_32x32x16_f16, 2^-22 relative per operand, with power-of-two
                              scales that keep every operand in f16 range: the NT per A row
                              (max_k |A[r,k]| < 2^E_r, A[r,:]·2^(14−E_r)) and per B column; the TN per
                              row block for A (from the NT's row_exp) and for G (a max|g| pass over
                              the block's rows).  Taken by the w1/w2 NT (N <= 128, k1, k2 multiples of
                              16, k1 + k2 <= 128, f32 A / C) and by the plain g-form TN given row_exp
                              (Nr % 4 == 0, 16-byte aligned g rows); any other call runs as
                              GNN_MATH_SPLIT_BF16 */
} gnn_gemm_math;
/* Skinny shapes run full-f32 VALU kernels whatever `math` says (the 2-class output layers,
 * gnn.py:23,66,124): NT with N <= 8 (K <= 384) or with K <= 8 (one A segment), f32 A/C and no
 * projection; TN with Nr <= 8 in the plain g form (no dz/proj, h or gout) and f32 A. */

typedef struct gnn_gemm_nt_params {
  int64_t M, N;                          /* C is [M, N] */
  const float* a1; int64_t lda1; int64_t k1;
  const float* a2; int64_t lda2; int64_t k2;   /* optional 2nd K segment: A = [A1 | A2] (k2 = 0: none) */
  const float* bt; int64_t ldb;          /* [k1+k2, N] row-major (Linear weight transposed), or NULL and: */
  const float* w1; const float* w2;      /* ... B read in place from PyTorch Linear weights W1 [N, k1], */
  int64_t ldw1, ldw2;                    /*     W2 [N, k2] (N <= 128): out = [A1|A2]·[W1|W2]ᵀ, no copy */
  float* c; int64_t ldc;                 /* output (may be NULL when only z is wanted) */
  const float* bias;                     /* [N] or NULL */
  int32_t relu;                          /* max(., 0) after bias */
  float dropout_p;                       /* after ReLU; 0 = off.  keep if hash(seed, row*N+col) < 1-p */
  uint64_t seed;                         /* per-call salt (the seed itself when seed_ptr is NULL) */
  const uint64_t* seed_ptr;              /* optional device counter: seed = *seed_ptr * golden + seed
                                            (graph-replay safe: bump the counter inside the graph) */
  const float* proj; int32_t nproj;      /* optional Z = C · projᵀ, proj [nproj, N], nproj <= 4, N <= 128 */
  float* z; int64_t ldz;
  int32_t math;                          /* gnn_gemm_math */
  void* workspace; size_t workspace_bytes; /* optional: the split-bf16 w1/w2 form pre-splits B here
                                            (gnn_gemm_nt_workspace_size) */
  int32_t a_dtype;                       /* gnn_dtype of A1/A2 (BF16: w1/w2 form; B rounded to bf16,
                                            one bf16 product, f32 accumulate — the bf16-storage path) */
  int32_t c_dtype;                       /* gnn_dtype of C (BF16 needs a_dtype BF16); z stays f32 */
  const float* mask;                     /* optional [M, N] (ldmask): C *= (mask > 0 ? mask_scale : 0)
                                            after the other epilogue steps — the ReLU + dropout
                                            backward of a saved activation (K <= 8 or N <= 8 shapes) */
  int64_t ldmask;
  float mask_scale;
  const void* a_planes;                  /* optional split image of [A1 | A2] (see gnn_split_planes_f32):
                                            A1 in columns [0, k1), A2 in [planes_col2, planes_col2 + k2),
                                            zeros elsewhere.  When the shape is one the split-image kernel
                                            takes (gnn_gemm_nt_planes_ok) A is read from it and a1 / a2 may
                                            be NULL; otherwise a1 / a2 are used (UNSUPPORTED if NULL). */
  int64_t planes_ld, planes_stride, planes_col2;
  int32_t planes_format;                 /* gnn_planes_format of a_planes (HALF_PAIR: 336-wide rows,
                                            1 <= N <= 128, N % 4 == 0; B per output column scaled by
                                            a power of two into f16 range, 3 f16 products) */
  const uint32_t* keep_mask;             /* optional (HALF_PAIR with dropout): the keep bits written by
                                            gnn_sage_mean_fwd_h2 for this call's seed / p / N; used
                                            instead of hashing every element in the epilogue */
  int32_t b_ready;                       /* image-A forms only: nonzero = workspace already holds the B
                                            image gnn_gemm_nt_prep_b wrote for these weights and shapes
                                            (the call launches only the GEMM) */
  int32_t planes_exp;                    /* HALF_PAIR (ABI 19): the image holds A * 2^planes_exp
                                            (gnn_split_h2_f32 scale_exp); C is unscaled exactly */
  float* colsum_part; int64_t colsum_cap; /* optional (ABI 21): the skinny-K form (k1 <= 8, k2 = 0,
                                            8 < N <= 256; UNSUPPORTED otherwise) also writes the column
                                            sums of the C it stores (after the whole epilogue), one row per
                                            block: colsum_part[b * N + n], b < gnn_gemm_nt_colsum_blocks;
                                            capacity colsum_cap floats.  gnn_colsum_finish_f32 then
                                            gives Σ_rows C — a layer's bias gradient without a pass over C */
  int32_t* row_exp;                      /* optional (ABI 23, GNN_MATH_HALF_PAIR form only): [M] per-row
                                            exponents E_r with max_k |[A1|A2][r,k]| < 2^E_r (0 for a zero
                                            row, 128 for a non-finite one) — the TN's A bound
                                            (gnn_gemm_tn_params.row_exp) for the same operand */
} gnn_gemm_nt_params;

/* C = epilogue([A1|A2] · Bt). */
gnn_status gnn_gemm_nt_colsum_blocks(const gnn_gemm_nt_params* p, int32_t* nb);  /* 0: no column sums */
gnn_status gnn_gemm_nt_workspace_size(int64_t N, int64_t k1, int64_t k2, size_t* bytes);
gnn_status gnn_gemm_nt_f32(const gnn_gemm_nt_params* p, gnn_stream_t stream);
/* The image-A forms' weight prep alone: writes the B image (split / half-pair / bf16 planes of
 * [w1 | w2]ᵀ, with the half-pair column scales) into p->workspace, for a later gnn_gemm_nt_f32 of
 * the same params with b_ready = 1.  Lets a caller run the prep on a second stream beside the
 * producer of A (it reads only the weights).  UNSUPPORTED (nothing launched) when the params do
 * not select an image-A kernel (gnn_gemm_nt_planes_ok). */
gnn_status gnn_gemm_nt_prep_b(const gnn_gemm_nt_params* p, gnn_stream_t stream);

typedef struct {
  int64_t M, Nr;                         /* dW is [Nr, k1+k2], Nr <= 128, k1+k2 <= 384 */
  const float* g; int64_t ldg;           /* G [M, Nr] ... */
  const float* dz; int64_t lddz;         /* ... or G = dz · proj (dz [M, nproj], proj [nproj, Nr]) */
  const float* proj; int32_t nproj;
  const float* h; int64_t ldh; float hscale;   /* optional: G *= (h > 0 ? hscale : 0) — ReLU+dropout bwd */
  float* gout; int64_t ldgout;           /* optional: store G */
  const float* a1; int64_t lda1; int64_t k1;
  const float* a2; int64_t lda2; int64_t k2;
  int32_t math;                          /* gnn_gemm_math */
  int32_t a_dtype;                       /* gnn_dtype of A1/A2 (BF16: G rounded to bf16, one product;
                                            needs M >= 16) */
  int32_t h_dtype;                       /* gnn_dtype of h */
  const void* a_planes;                  /* optional split image of [A1 | A2], as gnn_gemm_nt_params */
  int64_t planes_ld, planes_stride, planes_col2;
  int32_t planes_format;                 /* gnn_planes_format (HALF_PAIR: the dz form with h, 336-wide
                                            rows, or the plain g form over 336- / 176-wide rows; G scaled
                                            per row block by a power of two, 3 products) */
  int32_t g_dtype;                       /* gnn_dtype of g and gout (BF16: the bf16-image TN only; gout
                                            then holds the bf16-rounded G its MFMAs use) */
  int32_t planes_exp;                    /* HALF_PAIR (ABI 19): the image holds A * 2^planes_exp; dW is
                                            unscaled exactly */
  float* sq_partial;                     /* optional (ABI 20): the clip + Adam norm partials of `out`, for a
                                            call whose out holds every gradient of an optimizer group —
                                            per block b < nb of the ordered reduce (nb =
                                            gnn_gemm_tn_sq_blocks), over the out[j] with j outside
                                            [sq_skip_lo, sq_skip_hi): sq_partial[b] = Σ out[j]², sq_partial[nb + b]
                                            = the count of non-finite out[j]; sq_partial[2 nb] = *sq_step (the
                                            step count before the update).  Capacity sq_cap floats >= 2 nb + 1;
                                            hand them to gnn_clip_adam_f32 (gnn_adam_group.grad_sq_partial) */
  const float* sq_step;
  int64_t sq_skip_lo, sq_skip_hi, sq_cap;
  const int32_t* row_exp;                /* optional (ABI 23): [M] exponents bounding the rows of [A1|A2]
                                            (max_k |A[r,k]| < 2^row_exp[r]), as a GNN_MATH_HALF_PAIR NT of
                                            the same operand writes them; with math GNN_MATH_HALF_PAIR and
                                            the plain g form the TN runs in half-pair arithmetic */
  const uint32_t* g_rowmax;              /* optional (ABI 25), the plain g form over a half-pair image:
                                            [ceil(M / GNN_ROWMAX_ROWS)] float bits of max |G| over each
                                            group of GNN_ROWMAX_ROWS rows and all Nr columns (an upper
                                            bound is enough), as gnn_gat_bwd_act_proj_f32 writes them for
                                            its dxh: the TN takes its per-row-block power-of-two scale
                                            from these instead of a pass over its G rows.  Exact maxima
                                            give the scan's scale, so the result is bit-identical. */
  const gnn_graph* dz_graph;             /* optional (ABI 26), the half-pair dz form without gout: the TN
                                            itself forms dz[:, 0:dz_cols] = Σ over each row's CSC slots of
                                            dz_u[source, 0:dz_cols] — gnn_aggregate_f32(SUM, transpose) of
                                            dz_u, bit for bit — and writes it into dz before using it, so
                                            the caller skips that launch (the SAGE output layer's meanᵀ of
                                            u = dlogits / deg, gnn_sage_out_mean_ce_f32).  Inside its
                                            kernel when a row block is at most ~450 rows (a strong-scaling
                                            shard), else by that aggregation launched first.  1 <= dz_cols
                                            <= min(2, nproj), dz_graph->num_nodes == M; UNSUPPORTED outside
                                            that kernel.  gnn_gemm_tn_planes_ok returns 1 for such
                                            params only when the kernel forms the columns itself */
  const float* dz_u; int64_t ldu;
  int32_t dz_cols;
} gnn_gemm_tn_params;

/* Row-group granularity of gnn_gemm_tn_params.g_rowmax (ABI 25). */
#define GNN_ROWMAX_ROWS 16

/* Weight gradient dW = Gᵀ·[A1|A2] summed over all M rows (split-M slabs + ordered reduce).
 * out (contiguous): dW1 = Gᵀ·A1 [Nr, k1] | dW2 = Gᵀ·A2 [Nr, k2] | db = Σ_m G [Nr] |
 * (dz form) dWp = dzᵀ·h [nproj, Nr] | dzsum = Σ_m dz [nproj]. */
gnn_status gnn_gemm_tn_workspace_size(int64_t M, int64_t Nr, int64_t Kc, int32_t nproj, size_t* bytes);
gnn_status gnn_gemm_tn_f32(const gnn_gemm_tn_params* p, float* out, void* workspace, size_t workspace_bytes,
                           gnn_stream_t stream);
/* (ABI 28) gnn_gemm_tn_f32 over the row chunks whose dz can be nonzero.  dz_active: [ceil(M / 16)]
 * bytes, 16-byte aligned, one per GNN_ACTIVE_ROWS rows of dz; a 0 promises that every dz value of
 * the group is zero (gnn_aggregate_active_f32 writes such flags).  The half-pair dz form with h, no
 * gout and no dz_graph only, at every M >= 16 (never split-K): each row block of the dense call
 * walks only its flagged chunks, in order, so on a graph whose train rows sit in a few timesteps
 * most blocks finish at once and the rest stream A and h uncontended.  A skipped chunk would have
 * added exact zeros: the output is bit-identical to gnn_gemm_tn_f32 on the same operands, whatever
 * the flags, as long as they keep their promise.  Unflagged chunks of A and h are never read: a
 * non-finite value there no longer reaches the output (the dense product's 0 · NaN does).  Every
 * other form is refused with GNN_ERR_UNSUPPORTED before any launch.  dz_active NULL: exactly
 * gnn_gemm_tn_f32.
 * A gnn_gemm_tn_f32 call with dz_graph that launches the CSC sum itself (row blocks too large for
 * its kernel) takes the same route on its own when gnn_gemm_tn_active_pays(M), with flags kept
 * past the slabs of the workspace (gnn_gemm_tn_workspace_size counts them). */
gnn_status gnn_gemm_tn_active_f32(const gnn_gemm_tn_params* p, const uint8_t* dz_active, float* out,
                                  void* workspace, size_t workspace_bytes, gnn_stream_t stream);
/* 1 when the flags pay at M rows: the dz-form row block is larger than the in-kernel CSC fold takes
 * (more than 448 rows a block, M > 114,688) — a rule of M alone, so every route to the TN agrees. */
int gnn_gemm_tn_active_pays(int64_t M);
/* The flag-driven TN's launch form: each row block runs as gnn_gemm_tn_active_split() blocks, one per
 * contiguous range of 32-column k-tiles of the 336-wide image (11 tiles dealt as evenly as they go,
 * the longer ranges first), every block walking the same chunk list with the same scale into its
 * columns of the row block's one slab, with the loads of gnn_gemm_tn_active_ring() chunks in flight.
 * Row blocks without a flagged chunk write one word and the reduce skips their slabs.  None of it
 * changes a bit of the output.  Environment, read at every call (A/B): GNNMP_TN_ACTIVE_SPLIT=0 runs
 * one block per row block with one chunk of loads in flight, GNNMP_TN_EMPTY_SKIP=0 writes and reads
 * the zero slabs. */
int gnn_gemm_tn_active_split(void);
int gnn_gemm_tn_active_ring(void);
/* The number nb of norm partials a call with sq_partial writes for an out of n_out floats (ABI 20). */
gnn_status gnn_gemm_tn_sq_blocks(int64_t n_out, int32_t* nb);
/* 1 when the call would read A from p->a_planes (the f32 A operands are then not needed), else 0.
 * Split-image NT shapes (f32 C, the w1/w2 B form, N % 4 == 0, M >= 32; a ReLU, dropout or
 * projection epilogue needs relu + bias):
 *   image rows of 336 (the SAGE layer-1 [agg | x], 166 + 166 padded to 168 each), 64 < N <= 128;
 *   image rows of 176 (one input of <= 176 columns: the GCN / GAT layer-1 x), 1 <= N <= 128;
 *   a half-pair image (planes_format HALF_PAIR) of 336-wide rows, 1 <= N <= 128.
 * TN image rows of 32..336 (multiple of 16), f32 h; half-pair: the dz form with h, 336-wide rows,
 * or (ABI 19) the plain g form — g given, no dz / h / gout, 16-byte aligned g rows — over 336- or
 * 176-wide rows (gnn_gemm_tn_planes_ok).  Both need the planes to span < 2 GiB
 * and C / z below 2 GiB. */
int gnn_gemm_nt_planes_ok(const gnn_gemm_nt_params* p);
int gnn_gemm_tn_planes_ok(const gnn_gemm_tn_params* p);

/* ------------------------------------------------------------------------ */
/* Dense helpers used by the fused conv paths                               */
/* ------------------------------------------------------------------------ */
/* out[c] = sum_r x[r, c]  (bias gradients; deterministic two-stage column sum). */
gnn_status gnn_colsum_workspace_size(int64_t rows, int64_t F, size_t* bytes);
/* out[f] = Σ_b part[b * F + f] over b < nblk in gnn_colsum_f32's fixed order (ABI 21: the column
 * sums a skinny-K gnn_gemm_nt_f32 call wrote, gnn_gemm_nt_params.colsum_part) */
gnn_status gnn_colsum_finish_f32(const float* part, int32_t nblk, int64_t F, float* out, gnn_stream_t stream);
gnn_status gnn_colsum_f32(int64_t rows, int64_t F, const float* x, int64_t ldx, float* out,
                          void* workspace, size_t workspace_bytes, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K12 SAGEResBNNet layer tail, training mode (src/models/gnn.py:182-194):   */
/*     h = dropout(relu(BatchNorm1d(z))) + r,   r = res_proj(h_prev)          */
/* Replaces nn.BatchNorm1d.forward (batch statistics + running-stat update),  */
/* F.relu, F.dropout and the residual add, and their backward passes.         */
/* ------------------------------------------------------------------------ */
/* Workspace of gnn_bn_stats_f32 / gnn_bn_act_bwd_reduce_f32 for C channels. */
gnn_status gnn_bn_workspace_size(int64_t C, size_t* bytes);
/* Batch statistics of z [N, C]: stats (device float64 [2C + 1]) = [Σz | Σz² | N] — summable
 * across ranks (SyncBN: all-reduce them, then gnn_bn_finalize_f32).  finalize != 0 also does
 * gnn_bn_finalize_f32 in the same launch sequence (single device; with momentum >= 0 the merge
 * and the finalize are one launch).  N = 0 (an empty shard): with finalize == 0 stats is all zero
 * (n = 0), z may be null; with finalize != 0 an argument error (no batch mean). */
gnn_status gnn_bn_stats_f32(const float* z, int64_t ldz, int64_t N, int64_t C, double* stats, int32_t finalize,
                            float eps, float momentum, float* mean, float* invstd, float* running_mean,
                            float* running_var, int64_t* num_batches_tracked, void* workspace,
                            size_t workspace_bytes, gnn_stream_t stream);
/* mean = Σz/n, var = Σz²/n − mean² (biased, float64), invstd = 1/sqrt(var + eps); when
 * running_mean != NULL the nn.BatchNorm1d update: running = (1−m)·running + m·stat with the
 * unbiased variance, m = momentum (momentum < 0: PyTorch's momentum=None cumulative average
 * 1/(num_batches_tracked+1)), and num_batches_tracked += 1 (optional pointer). */
gnn_status gnn_bn_finalize_f32(const double* stats, int64_t C, float eps, float momentum, float* mean,
                               float* invstd, float* running_mean, float* running_var,
                               int64_t* num_batches_tracked, gnn_stream_t stream);
/* h = dropout(relu((z − mean)·invstd·weight + bias)) + r   (r optional; counter-hash dropout of
 * element r·C + c as gnn_agg_params; N·C < 2^32). */
gnn_status gnn_bn_act_res_fwd_f32(const float* z, int64_t ldz, const float* r, int64_t ldr, int64_t N, int64_t C,
                                  const float* mean, const float* invstd, const float* weight, const float* bias,
                                  float dropout_p, uint64_t seed, const int64_t* seed_ptr, float* h, int64_t ldh,
                                  gnn_stream_t stream);
/* Backward, step 1: sums (device float [2C]) = [Σ dy | Σ dy·x̂] over the N rows, with
 * dy = dh ⊙ dropout-mask/(1−p) ⊙ [y > 0] recomputed from z (the BN weight / bias gradients are
 * these local sums; SyncBN all-reduces a copy before step 2). */
gnn_status gnn_bn_act_bwd_reduce_f32(const float* dh, int64_t lddh, const float* z, int64_t ldz, int64_t N,
                                     int64_t C, const float* mean, const float* invstd, const float* weight,
                                     const float* bias, float dropout_p, uint64_t seed, const int64_t* seed_ptr,
                                     float* sums, void* workspace, size_t workspace_bytes, gnn_stream_t stream);
/* Backward, step 2: dz = weight·invstd·(dy − Σdy/n − x̂·Σdy·x̂/n) with the (global) sums and the
 * device row count *n_total (stats[2C] of the forward; torch.batch_norm_backward_elemt). */
gnn_status gnn_bn_act_bwd_f32(const float* dh, int64_t lddh, const float* z, int64_t ldz, int64_t N, int64_t C,
                              const float* mean, const float* invstd, const float* weight, const float* bias,
                              float dropout_p, uint64_t seed, const int64_t* seed_ptr, const float* sums,
                              const double* n_total, float* dz, int64_t lddz, gnn_stream_t stream);
/* The same, also writing the column sums of the dz it stores per block, colsum[b·C + c] for
 * b < gnn_bn_act_bwd_colsum_blocks(N, C) (N >= 1, C <= 256; ABI 21): the bias gradient of the
 * conv that produced z, through gnn_colsum_finish_f32, without a pass over dz. */
gnn_status gnn_bn_act_bwd_colsum_blocks(int64_t N, int64_t C, int32_t* nb);
gnn_status gnn_bn_act_bwd_colsum_f32(const float* dh, int64_t lddh, const float* z, int64_t ldz, int64_t N, int64_t C,
                                     const float* mean, const float* invstd, const float* weight, const float* bias,
                                     float dropout_p, uint64_t seed, const int64_t* seed_ptr, const float* sums,
                                     const double* n_total, float* dz, int64_t lddz, float* colsum,
                                     gnn_stream_t stream);

/* K13: SAGEResBNNet's input with the fixed sinusoid time features, out = [x | te(t)] in one pass
 * (replaces SAGEResBN._time_embed / torch.cat of src/models/gnn.py:145-160, 172-176):
 * te_k = sin(t·2π(k+1)) for k < dim/2, cos(t·2π(k-dim/2+1)) for k < 2·(dim/2), 0 after, with
 * t = clamp(t_idx - 1, 0, T - 1) / max(T - 1, 1) (T = max_timestep).  x [N, F] (ldx), t_idx int64
 * [N], out [N, F + dim] (ldo).  No gradient: the features carry no parameters. */
gnn_status gnn_time_inject_sin_f32(const float* x, int64_t ldx, int64_t N, int64_t F, const int64_t* t_idx,
                                   int64_t dim, int64_t max_timestep, float* out, int64_t ldo, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Step ops around the hot path (src/train_gnn.py:136-183, 201-206)          */
/* ------------------------------------------------------------------------ */
/* Masked class-weighted cross entropy over all N rows, forward and backward in one pass:
 * rows with mask[i] != 0 and 0 <= y[i] < C contribute loss_i = -w[y_i]·log_softmax(x_i)[y_i]
 * (F.cross_entropy(weight=w, reduction='none')); *loss = Σ loss_i · inv_denom (the reference's
 * loss_vec.mean() with inv_denom = 1 / n_train, src/train_gnn.py:175); dlogits = d(*loss)/dx
 * (zero on every other row).  C <= 16.  Deterministic fixed-order reduction. */
gnn_status gnn_masked_ce_workspace_size(int64_t N, size_t* bytes);
/* loss = NULL (ABI 18): the per-block partial sums stay in the workspace (its first ceil(N / 256)
 * floats) and the loss is finished later — by gnn_masked_ce_finish, or inside a gnn_clip_adam_f32
 * call (gnn_adam_group.loss_partial) when nothing reads it before the optimizer (a captured step). */
gnn_status gnn_masked_ce_finish(const float* partial, int32_t nblk, float inv_denom, float* loss, gnn_stream_t stream);
/* gnn_masked_ce_f32 (N >= 1) that also writes the per-256-row-block column sums of dlogits,
 * colsum[b * C + c], b < ceil(N / 256) (ABI 21): gnn_colsum_finish_f32(colsum, ceil(N / 256), C, db)
 * is then the output layer's bias gradient without a pass over dlogits. */
/* GCN's output layer and the masked CE in one launch (ABI 21): logits = Â·t + bias (gnn_aggregate_f32
 * GCN over a LOOPS_REPLACE plan, dinv = gnn_gcn_norm_f32, 1 <= C <= 2) and gnn_masked_ce_f32 of
 * them with its workspace contract (loss NULL: partials deferred); colsum (optional): the
 * per-256-row-block column sums of dlogits as gnn_masked_ce_colsum_f32 writes them. */
gnn_status gnn_gcn_out_ce_f32(const gnn_graph* g, const float* dinv, const float* t, int64_t ldt, int32_t C,
                              const float* bias, float* logits, int64_t ldo, const int64_t* y, const uint8_t* mask,
                              const float* class_w, float inv_denom, float* dlogits, int64_t ld_d, float* colsum,
                              float* loss, void* workspace, size_t workspace_bytes, gnn_stream_t stream);
gnn_status gnn_masked_ce_colsum_f32(int64_t N, int32_t C, const float* logits, int64_t ldx, const int64_t* y,
                                    const uint8_t* mask, const float* class_w, float inv_denom, float* dlogits,
                                    int64_t ld_d, float* loss, void* workspace, size_t workspace_bytes,
                                    float* colsum, gnn_stream_t stream);
gnn_status gnn_masked_ce_f32(int64_t N, int32_t C, const float* logits, int64_t ldx, const int64_t* y,
                             const uint8_t* mask, const float* class_w, float inv_denom, float* dlogits,
                             int64_t ld_d, float* loss, void* workspace, size_t workspace_bytes,
                             gnn_stream_t stream);

/* The masked CE's loss variants (ABI 27; src/train_gnn.py:136-183): one description of the loss for
 * every CE entry point, so a new variant is a field here and not an argument of each of them.
 *   base_i = focal ? -(1 - p)^gamma · log p          (no class weight: the reference's focal drops it)
 *                  : -class_w[y_i] · log p           (p = softmax(x_i)[y_i])
 *   loss_i = row_w[i] · base_i                       (row_w NULL: 1; the time weighting, built by the host)
 *   *loss  = Σ loss_i · inv_denom,  dlogits = d(*loss)/dx
 * on rows with mask[i] != 0 and 0 <= y[i] < C, zero elsewhere.  1 - p is formed from the other
 * classes' exponentials, so it keeps its relative accuracy as p -> 1; gamma 1 and 2 are plain
 * products ((1 - p)^0 = 1 also at p = 1).  focal with gamma < 1 is GNN_ERR_INVALID_ARG: its
 * gradient is unbounded at p = 1.  row_w = NULL, focal = 0 is exactly the entry point without
 * _spec (the same kernel, bit for bit).  reserved: zero. */
typedef struct {
  const int64_t* y;       /* [N] labels */
  const uint8_t* mask;    /* [N] row mask */
  const float* class_w;   /* [C] class weights (never NULL; the focal loss does not apply them) */
  const float* row_w;     /* [N] per-row weights, or NULL */
  float inv_denom;
  int32_t focal;          /* 0 / 1 */
  float focal_gamma;      /* >= 1 when focal */
  int32_t reserved[5];
} gnn_ce_spec;

/* gnn_masked_ce_f32 / gnn_masked_ce_colsum_f32 (colsum optional here; with it N >= 1) of a spec. */
gnn_status gnn_masked_ce_spec_f32(int64_t N, int32_t C, const float* logits, int64_t ldx, const gnn_ce_spec* spec,
                                  float* dlogits, int64_t ld_d, float* loss, void* workspace,
                                  size_t workspace_bytes, float* colsum, gnn_stream_t stream);
/* gnn_sage_out_mean_ce_f32, gnn_gcn_out_ce_f32 and gnn_gat_out_ce_f32 of a spec (spec NULL in the
 * GAT form: no CE), each with the C limits and the u / colsum / loss / workspace contract of the
 * entry point it stands beside; the results equal that layer's own launch followed by
 * gnn_masked_ce_spec_f32 bit for bit. */
gnn_status gnn_sage_out_mean_ce_spec_f32(const gnn_graph* g, const float* deg, const float* z, int64_t ldz,
                                         int32_t C, const float* bias, float* logits, int64_t ldo,
                                         const gnn_ce_spec* spec, float* dlogits, int64_t ld_d, float* u,
                                         int64_t ldu, float* colsum, float* loss, void* workspace,
                                         size_t workspace_bytes, gnn_stream_t stream);
gnn_status gnn_gcn_out_ce_spec_f32(const gnn_graph* g, const float* dinv, const float* t, int64_t ldt, int32_t C,
                                   const float* bias, float* logits, int64_t ldo, const gnn_ce_spec* spec,
                                   float* dlogits, int64_t ld_d, float* colsum, float* loss, void* workspace,
                                   size_t workspace_bytes, gnn_stream_t stream);
gnn_status gnn_gat_out_ce_spec_f32(const gnn_graph* g, const gnn_gat_fwd_params* p, const gnn_ce_spec* spec,
                                   float* dlogits, int64_t ld_d, float* colsum, float* loss, void* workspace,
                                   size_t workspace_bytes, gnn_stream_t stream);

/* clip_grad_norm_(max_norm) + torch.optim.Adam.step() (weight_decay as L2 on the gradient) over
 * up to GNN_ADAM_MAX_TENSORS parameters (src/train_gnn.py:203-206).  `step` is a device float
 * incremented by the call (graph-replay safe); norm_out (optional, device) gets the pre-clip
 * total norm.  max_norm <= 0 disables clipping.  Grads are scaled in place, as torch does. */
#define GNN_ADAM_MAX_TENSORS 24
typedef struct {
  float* param; float* grad; float* exp_avg; float* exp_avg_sq; int64_t numel;
} gnn_adam_tensor;
typedef struct {
  int32_t num_tensors;
  double lr, beta1, beta2, eps, weight_decay, max_norm;  /* double, as torch's Python scalars */
  gnn_adam_tensor tensors[GNN_ADAM_MAX_TENSORS];
  int32_t skip_nonfinite;  /* != 0: torch.amp.GradScaler.step semantics — any inf / NaN gradient
                              ELEMENT skips the update (params, moments, grads and step count
                              untouched); finite gradients whose Σg² overflows are clipped by
                              coefficient 0, as clip_grad_norm_ does with an inf norm */
  int64_t* bump_counter;   /* optional (ABI 18): a device int64 the call increments by one (the
                              dropout seed counter of a captured step — gnn_gemm_nt_params.seed_ptr
                              — advanced at the step's end instead of by a launch of its own) */
  const float* loss_partial; int32_t loss_nblk; float loss_scale; float* loss_out;
                           /* optional (ABI 18): *loss_out = loss_scale · Σ loss_partial[0 .. loss_nblk)
                              in gnn_masked_ce_f32's order — the loss of a gnn_masked_ce_f32 call made
                              with loss = NULL, finished in this call */
  const float* grad_sq_partial; int32_t grad_sq_nblk;
                           /* optional (ABI 20): the norm partials a gnn_gemm_tn_f32 call wrote
                              (gnn_gemm_tn_params.sq_partial, nb = grad_sq_nblk) for EXACTLY these
                              tensors' gradients, with *step as sq_step: the call then launches only the
                              clip + Adam kernel (its Σg² pass is folded into the TN's reduce) */
} gnn_adam_group;
/* Workspace: 2·64 + 2 words, ZEROED before the first call.  Without grad_sq_partial, gradients of
 * at most 2^15 elements in all (GCN, GAT of the path) run as ONE launch: each block sums Σg² over
 * all of them itself, in one fixed order, and the last block to finish advances *step (a vector
 * atomic on the workspace's last word, a running count: each call adds exactly 64 and the block
 * that draws 63 mod 64 is the last, so a call that never completed cannot leave later calls
 * without a last block — no reset is needed, re-zeroing the workspace is always safe between
 * calls); larger ones run the Σg² pass first (two launches).  ABI 21. */
gnn_status gnn_clip_adam_workspace_size(size_t* bytes);
gnn_status gnn_clip_adam_f32(const gnn_adam_group* group, float* step, float* norm_out, void* workspace,
                             size_t workspace_bytes, gnn_stream_t stream);
/* (additive to ABI 32) gnn_clip_adam_f32 that also builds, in the same launch, the B images of
 * num_nts (1 .. 4) half-pair NTs from the weights it has just updated: nts[i] are the params of
 * those NT calls as gnn_gemm_nt_prep_b takes them (w1 / w2, the image fields, the B workspace).
 * Afterwards each workspace holds exactly what gnn_gemm_nt_prep_b(&nts[i]) would write for the
 * updated weights, so the next NT over them runs with b_ready = 1 and no prep launch.  The
 * update is bit for bit gnn_clip_adam_f32's (params, moments, clipped grads, *step, norm_out).
 * A step skipped under skip_nonfinite leaves the weights alone and builds the image of the
 * unchanged weights.  Refused with GNN_ERR_INVALID_ARG before any launch: an nts[i] that does
 * not select the half-pair NT (its shapes, a large enough workspace); w1 (or w2 when k2 > 0) that
 * is not the `param` of a group tensor of N·k elements, or is claimed twice; ldw != k; a group
 * that runs the one-launch form (no grad_sq_partial and at most 2^15 elements).  Every gradient,
 * moment and parameter element keeps exactly one writer; no block waits for another. */
gnn_status gnn_clip_adam_prep_f32(const gnn_adam_group* group, float* step, float* norm_out, void* workspace,
                                  size_t workspace_bytes, const gnn_gemm_nt_params* nts, int32_t num_nts,
                                  gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K11 NeighborLoader neighbour sampling (torch_geometric.loader.NeighborLoader + pyg-lib
 *     neighbor_sample, built at src/train_gnn.py:329-348 and consumed by
 *     train_epoch_minibatch / eval_val_minibatch, src/train_gnn.py:212-276)            */
/* ------------------------------------------------------------------------ */
/* Workspace for gnn_neighbor_sample over a graph of num_nodes with the given capacities. */
gnn_status gnn_neighbor_sample_workspace_size(int64_t num_nodes, int64_t node_cap, int64_t edge_cap,
                                              size_t* bytes);

/* Sample one batch over the CSR-by-target direction of `g` (a GNN_LOOPS_KEEP plan of the
 * full graph's edge_index): seeds[num_seeds] (distinct, device int32) become local nodes
 * 0..B-1; hop h samples up to fanout[h] (host array; -1 = all, else >= 1) in-neighbours of
 * every node first discovered in hop h-1, uniformly without replacement (all of them when the
 * in-degree is <= fanout), from a counter hash of (seed, hop, node, draw).  New nodes are
 * appended to n_id in order of first appearance in the hop's edge list (disjoint=False dedup).
 * Edges: e_src[s] -> e_dst[s] in local ids (the original edge direction), e_id[s] = PyG edge
 * id (csr_eid[slot], or the CSR slot when csr_eid is NULL); hop-major, then frontier node,
 * then PyG edge order.  hop_nodes[num_hops+1] / hop_edges[num_hops] (HOST arrays) receive
 * PyG's num_sampled_nodes / num_sampled_edges.  Output sizes are data dependent: the call
 * synchronises `stream` twice per hop to read them.  INVALID_ARG when a capacity is exceeded
 * or seeds repeat, INDEX_OUT_OF_RANGE for a seed outside [0, N). */
gnn_status gnn_neighbor_sample(const gnn_graph* g, const int32_t* csr_eid, const int32_t* seeds,
                               int64_t num_seeds, int32_t num_hops, const int32_t* fanout, uint64_t seed,
                               int32_t* n_id, int64_t node_cap, int32_t* e_src, int32_t* e_dst,
                               int32_t* e_id, int64_t edge_cap, int64_t* hop_nodes, int64_t* hop_edges,
                               void* workspace, size_t workspace_bytes, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K14 ranking metrics (ABI 29): sklearn.metrics.average_precision_score as src/utils/metrics.py:10-12
 *     calls it, the per-timestep loop of src/train_gnn.py:497-519, precision_at_k
 *     (metrics.py:37-39) and the replicates of src/analysis/bootstrap_compare.py          */
/* ------------------------------------------------------------------------ */
#define GNN_RANK_TILE 1024               /* order positions per block of the AP scan */
#define GNN_RANK_BOOT_LDS_MAX_N 32768    /* bootstrap: n up to this histograms in LDS, above in global memory */
/* bits of the device status word (OR-ed in by the calls; the caller zeroes and reads it) */
#define GNN_RANK_STATUS_NAN 1            /* an included score is NaN */
#define GNN_RANK_STATUS_SEGMENT 2        /* an included element's segment is outside [0, S): it was excluded */
#define GNN_RANK_STATUS_INDEX 4          /* a bootstrap sample index is outside [0, n), or a plan is not whole */

/*
 * Rank plan of scores[n] (f32): order[n] holds the included elements (include[i] != 0; NULL = all)
 * sorted by (segment ascending, score descending, index ascending) — segment[i] in [0, S), NULL =
 * one segment — followed by the excluded ones; seg_ptr[S+1] the segments' first positions with
 * seg_ptr[S] = m, the number of included elements (it stays on the device); flags[n] per position:
 * bit 0 last of its tie group (bit-equal scores of one segment; -0.0 == +0.0), bit 1 first of its
 * segment, bit 2 first of its tie group; rank[n] (optional) the inverse of order.  One stable radix
 * sort of 64-bit (segment, inverted orderable score) keys over the bits in use.
 */
gnn_status gnn_rank_plan_workspace_size(int64_t n, int64_t num_segments, size_t* bytes);
gnn_status gnn_rank_plan_build(const float* scores, const uint8_t* include, const int32_t* segment,
                               int64_t n, int64_t num_segments, int32_t* order, uint8_t* flags,
                               int32_t* seg_ptr, int32_t* rank, int32_t* status, void* workspace,
                               size_t workspace_bytes, gnn_stream_t stream);

/*
 * Per segment s of a plan: ap[s] = sum over tie groups g of (TP_g - TP_{g-1}) * TP_g / (TP_g + FP_g),
 * over P (f64; 0 when P = 0 or the segment is empty), num_pos[s] = P, count[s] = elements, and with
 * patk (optional; needs k >= 1) the mean of positive[] over the first min(k, count[s]) positions.
 * positive[n] is indexed by element (non-zero = positive).  Integer counts, f64 terms summed in one
 * fixed order: bitwise reproducible.
 */
gnn_status gnn_rank_ap_workspace_size(int64_t n, int64_t num_segments, size_t* bytes);
gnn_status gnn_rank_ap(const int32_t* order, const uint8_t* flags, const int32_t* seg_ptr,
                       const uint8_t* positive, int64_t n, int64_t num_segments, int64_t k, double* ap,
                       int64_t* num_pos, int64_t* count, double* patk, void* workspace,
                       size_t workspace_bytes, gnn_stream_t stream);

/*
 * Paired bootstrap replicates: plans A and B of two score vectors over the same n elements (no mask,
 * one segment) and sample_idx[num_replicates, n] (int32 in [0, n)).  Replicate r weighs element i by
 * how often row r draws it; ap_x[r] is the weighted average precision (equal to the AP of the
 * resampled arrays) and patk_x[r] the weighted precision at k (min(w_i, k - taken) copies per element
 * in plan order).  num_replicates < 65536 per call; k >= 1.  n <= GNN_RANK_BOOT_LDS_MAX_N needs no
 * workspace beyond the queried minimum.
 */
gnn_status gnn_rank_bootstrap_workspace_size(int64_t n, int64_t num_replicates, size_t* bytes);
gnn_status gnn_rank_bootstrap(const int32_t* order_a, const int32_t* rank_a, const uint8_t* flags_a,
                              const int32_t* order_b, const int32_t* rank_b, const uint8_t* flags_b,
                              const uint8_t* positive, const int32_t* sample_idx, int64_t n,
                              int64_t num_replicates, int64_t k, double* ap_a, double* ap_b,
                              double* patk_a, double* patk_b, int32_t* status, void* workspace,
                              size_t workspace_bytes, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K15 seeded input perturbations (ABI 30): drop_edges and maybe_add_noise of
 *     src/analysis/robustness.py:65-90, from a counter hash with a bit-exact host mirror
 *     (elliptic_gnn_project_amd/robustness.py) in place of torch.randperm / torch.randn_like   */
/* ------------------------------------------------------------------------ */
/*
 * H(c, key) = fmix32(((uint32)c * 0x9E3779B1 + key_lo) ^ key_hi) (the dropout mask's hash), and
 * stream_key(seed, s) = splitmix64(seed ^ (s * 0xD1B54A32D192ED03)); streams: 1 edge drop, 2 noise
 * radius, 3 noise angle.
 *
 * gnn_edge_drop: out[2, E - drop_count] = edge_index[2, E] (contiguous int64) without the drop_count
 * columns e of smallest (H(e, key), e), the kept columns in their original order; key is
 * stream_key(seed, 1), formed by the caller.  drop_count must lie in [0, num_edges) (INVALID_ARG
 * otherwise; num_edges = 0 with drop_count = 0 is a no-op); drop_count = 0 launches nothing and leaves
 * `out` untouched.  The output size is known to the caller: no host synchronisation, capturable.
 */
gnn_status gnn_edge_drop_workspace_size(int64_t num_edges, size_t* bytes);
gnn_status gnn_edge_drop(const int64_t* edge_index, int64_t num_edges, int64_t drop_count, uint64_t key,
                         int64_t* out, void* workspace, size_t workspace_bytes, gnn_stream_t stream);

/*
 * out[row, col] = x[row, col] + noise_std * z(row, col) over [rows, F] f32 (out may be x).  With
 * P = ceil(F / 2) and c = row * P + col / 2 (one Box-Muller pair per two neighbouring columns):
 *   u1 = ((H(c, stream_key(key, 2)) >> 8) + 1) * 2^-24,   u2 = (H(c, stream_key(key, 3)) >> 8) * 2^-24,
 *   r = sqrt(-2 ln u1),   z = r cos(2 pi u2) for even col, r sin(2 pi u2) for odd col;   |z| <= 5.77.
 * `key` is the call's 64-bit seed; the two stream keys are derived from it on the host.  16-byte
 * accesses when both bases are 16-byte aligned and both leading dimensions multiples of 4, 8-byte
 * ones for 8 / 2, else element accesses.  rows = 0 or F = 0 launches nothing.  INVALID_ARG for a
 * leading dimension below F or rows * P >= 2^32 (the counter is 32 bits wide).
 */
gnn_status gnn_feature_noise_f32(const float* x, int64_t ldx, int64_t rows, int64_t F, float noise_std,
                                 uint64_t key, float* out, int64_t ldo, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K16 fused GNNExplainer mask step (ABI 31): the per-epoch update of one mask of PyG 2.5.3
 *     GNNExplainer (src/analysis/explain.py:593-672 drives it) in one launch: the hard-entry
 *     size and entropy regularisers' gradient, torch.optim.Adam's step and, for the node-feature
 *     mask, the sigmoid gate's backward and the next forward's h = x * sigmoid(mask)           */
/* ------------------------------------------------------------------------ */
#define GNN_EXPLAIN_STATUS_BLOCK 1 /* a block id outside [0, num_blocks): that row / element was skipped */

/*
 * One mask of logits.  Plain form (x == NULL; the edge mask): mask, grad, exp_avg, exp_avg_sq,
 * hard / hard_out and block_of are [n] arrays (F and every leading dimension are ignored) and `grad`
 * is the autograd gradient wrt the logits.  Gate form (x != NULL; the node-feature mask): [n, F]
 * matrices with leading dimensions (elements), block_of[n] per row, and the gradient is
 * dh * x * s * (1 - s) with s = sigmoid(mask) and dh the gradient wrt h = x * s.
 *
 *   g = grad + hard * s (1 - s) (size_scale[b] + ent_scale[b] * (-log(s + EPS) - s / (s + EPS)
 *                                               + log(1 - s + EPS) + (1 - s) / (1 - s + EPS)))
 * with b = block_of[.], EPS = 1e-15 and 1 - s evaluated as sigmoid(-mask); then torch.optim.Adam's
 * step t (>= 1) on mask / exp_avg / exp_avg_sq: exp_avg = beta1 exp_avg + (1 - beta1) g,
 * exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g^2, mask -= lr / (1 - beta1^t) * exp_avg /
 * (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps).  hard == NULL is epoch 0: no regulariser
 * (size_scale / ent_scale may be NULL) and hard_out = (grad != 0) is written.  The gate form then
 * writes h = x * sigmoid(mask) from the updated logits when h != NULL.  t == 0 (gate form only)
 * updates nothing and only writes h.
 *
 * A row / element whose block id lies outside [0, num_blocks) is left untouched and sets
 * GNN_EXPLAIN_STATUS_BLOCK in *status (a plain store of the bit; the caller zeroes and reads the
 * word).  16-byte accesses when every f32 base is 16-byte aligned and every leading dimension a
 * multiple of 4 (the byte masks: 4-byte aligned), 8-byte ones for 8 / 2, else element accesses; the
 * last partial group of a row goes element by element.  Elementwise, no atomics: bitwise
 * reproducible.  n = 0 or (gate form) F = 0 launches nothing.  INVALID_ARG before any launch: a
 * leading dimension below F, t < 0, t == 0 in the plain form or without h, num_blocks < 1, n or F
 * negative, or a missing mask / grad (dh, x) / moment / block_of / status / hard_out (epoch 0) /
 * scale (later epochs) pointer.
 */
typedef struct {
  int64_t n;                /* elements (plain form) or rows (gate form) */
  int64_t F;                /* gate form: columns */
  float* mask;              /* logits, updated in place */
  int64_t ld_mask;
  const float* grad;        /* plain form: d loss / d mask */
  const float* dh;          /* gate form: d loss / d h */
  int64_t ld_dh;
  const float* x;           /* gate form: the gated features */
  int64_t ld_x;
  float* h;                 /* gate form, optional: x * sigmoid(updated mask) */
  int64_t ld_h;
  float* exp_avg;           /* Adam moments, shaped as mask, sharing ld_state */
  float* exp_avg_sq;
  int64_t ld_state;
  const uint8_t* hard;      /* hard mask (non-zero = hard); NULL: epoch 0 */
  uint8_t* hard_out;        /* epoch 0: receives grad != 0 */
  int64_t ld_hard;          /* of hard and hard_out */
  const int32_t* block_of;  /* [n] block of each element / row */
  int32_t num_blocks;       /* B >= 1 */
  int32_t t;                /* Adam step count of this call, 1-based; 0: only write h */
  const float* size_scale;  /* [B] coefficient of sum s over the block's hard entries */
  const float* ent_scale;   /* [B] coefficient of sum ent(s) over the block's hard entries */
  double lr, beta1, beta2, eps; /* torch.optim.Adam's; 1 - beta and the bias corrections are formed in double */
  int32_t* status;          /* device status word */
} gnn_explain_step_params;

gnn_status gnn_explain_mask_step_f32(const gnn_explain_step_params* p, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K17 device evaluation (ABI 32): TemperatureScaler.fit (src/utils/calibrate.py:8-30) as the
 *     minimiser of the validation NLL, and the host metrics of src/utils/metrics.py:14-66
 *     (ROC-AUC, max-F1 / precision-target threshold, F1 at a threshold, recall at precision,
 *     ECE) on the device.  Nothing synchronises or allocates; every call is capturable.       */
/* ------------------------------------------------------------------------ */
#define GNN_FIT_THREADS 1024             /* the temperature fit's one workgroup */
/* bits of the fit's device status word (OR-ed in; the caller zeroes and reads it) */
#define GNN_FIT_STATUS_LABEL 1           /* an included row's label is outside {0, 1}: it was skipped */
#define GNN_FIT_STATUS_NAN 2             /* an included row has a NaN or infinite logit: it was skipped */
#define GNN_FIT_STATUS_EMPTY 4           /* no row to fit: T = 1 */
#define GNN_FIT_STATUS_FLAT 8            /* |g(1)| <= 1e-7: T = 1 exactly (LBFGS's tolerance_grad exit) */
#define GNN_FIT_STATUS_CLAMP_LOW 16      /* g(2^-10) >= 0: beta = 2^-10 (T = 1024) */
#define GNN_FIT_STATUS_CLAMP_HIGH 32     /* g(2^10) <= 0: beta = 2^10 */
#define GNN_FIT_STATUS_MAXIT 64          /* 100 Newton updates without meeting the step tolerance */
#define GNN_CURVE_OUTPUTS 8              /* doubles gnn_rank_curve writes */
#define GNN_CALIB_MAX_BINS 32            /* most calibration bins of gnn_threshold_calibration */

/*
 * Temperature of two-class logits[n, 2] (f32, row stride ld >= 2 elements) against y[n] (int64) over
 * the rows with include[i] != 0 (NULL: the rows with y in {0, 1}).  An included row with another label
 * sets GNN_FIT_STATUS_LABEL, one with a NaN or infinite logit GNN_FIT_STATUS_NAN; both are skipped.
 * With m_i = (double)z[i, y_i] - (double)z[i, 1 - y_i] over the remaining rows and beta = 1 / T, in f64
 * with sigma and softplus evaluated through exp(-|t|):
 *   f(beta) = mean softplus(-beta m_i)     g = -mean m_i sigma(-beta m_i)
 *   h = mean m_i^2 sigma(beta m_i) sigma(-beta m_i)
 * Rules, in order: no row -> T = 1, EMPTY; |g(1)| <= 1e-7 -> T = 1, FLAT; g(2^-10) >= 0 -> beta = 2^-10,
 * CLAMP_LOW; g(2^10) <= 0 -> beta = 2^10, CLAMP_HIGH; else Newton from beta = 1 inside the bracket
 * g(lo) < 0 < g(hi): the candidate beta - g / h, or the bracket's midpoint when h == 0 or the candidate
 * is not strictly inside; stop at g == 0, at |beta_new - beta| <= 2^-40 beta (beta_new is kept; a Newton
 * step |g / h| <= 2^-40 beta stops too, keeping its candidate when strictly inside and beta otherwise), or
 * after 100 updates (MAXIT).  T[1] (f32) = (float)(1 / beta); diag[4] (f64) = {beta, f(beta), g(beta),
 * updates made}.  One workgroup of GNN_FIT_THREADS does all of it in one launch: the margins are
 * compacted into the workspace in row order and every sum runs in one fixed order (bitwise
 * reproducible).  Workspace: n doubles.  INVALID_ARG before any launch: n < 0, ld < 2, a missing T /
 * diag / status (or, with n > 0, logits / y); WORKSPACE for a short one.
 */
gnn_status gnn_temperature_fit_workspace_size(int64_t n, size_t* bytes);
gnn_status gnn_temperature_fit(const float* logits, int64_t ld, const int64_t* y, const uint8_t* include,
                               int64_t n, float* T, double* diag, int32_t* status, void* workspace,
                               size_t workspace_bytes, gnn_stream_t stream);

/*
 * Curve metrics of ONE-segment plan (gnn_rank_plan_build with num_segments = 1; any other value is
 * INVALID_ARG) over positive[n] (by element) and scores[n] (the plan's scores, to report thresholds).
 * P / N the included positives / negatives; at the end of tie group g with cumulative TP, FP and the
 * group's own gTP, gFP: prec = TP / (TP + FP), rec = TP / P (1.0 when P = 0) and
 * f1 = 2.0 * prec * rec / (prec + rec + 1e-12), each operation rounded in f64 in that order.
 * out[GNN_CURVE_OUTPUTS] (f64):
 *   [0] max-F1 threshold: the score of the group of largest f1, the lowest score among equals (1.0
 *       without a group)                                  [1] that f1 (0.0 without a group)
 *   [2] precision-target threshold: the lowest score among groups with prec >= target_precision; without
 *       one, 1.0 when 1 >= target_precision, else out[0]
 *   [3] recall at precision: the largest rec among groups with prec >= target_precision, 0.0 without one
 *   [4] ROC-AUC = sum_g gFP (2 TP - gTP) / (2 P N): an int64 sum and one f64 division; NaN when P or N is 0
 *   [5] P   [6] N   [7] the included elements
 * The argmax reductions compare (value, position) exactly: bitwise reproducible whatever their order.
 */
gnn_status gnn_rank_curve_workspace_size(int64_t n, size_t* bytes);
gnn_status gnn_rank_curve(const int32_t* order, const uint8_t* flags, const int32_t* seg_ptr,
                          const uint8_t* positive, const float* scores, int64_t n, int64_t num_segments,
                          double target_precision, double* out, void* workspace, size_t workspace_bytes,
                          gnn_stream_t stream);

/*
 * One pass over scores[n] (f32), positive[n], include[n] (NULL = all), no sort: counts[3] (int64) =
 * TP, FP, FN of (double)score >= thr; per bin b of the `bins` (1 .. GNN_CALIB_MAX_BINS) bins given by
 * edges[bins + 1] (HOST array, ascending f64, read during the call), with
 * bin = clip(#{edges <= (double)score} - 1, 0, bins - 1) (numpy's searchsorted side="right"):
 * bin_count[b], bin_pos[b] (int64) and bin_sum[b] = sum of (double)score (f64, one fixed order).
 * out[2] (f64) = {f1 = 2 TP / (2 TP + FP + FN) (0 when the denominator is 0),
 * ece = sum over non-empty bins of bin_count / n * |bin_pos / bin_count - bin_sum / bin_count|}.
 * thr must be a float32 value (every threshold of the pipeline is a score or 1.0; numpy's f32
 * comparison and this f64 one then agree).  INVALID_ARG before any launch: n < 0, bins out of range,
 * a missing pointer, thr not a float32 value, descending edges; WORKSPACE for a short one.
 */
gnn_status gnn_threshold_calibration_workspace_size(int64_t n, int32_t bins, size_t* bytes);
gnn_status gnn_threshold_calibration(const float* scores, const uint8_t* positive, const uint8_t* include,
                                     int64_t n, double thr, const double* edges, int32_t bins,
                                     int64_t* counts, int64_t* bin_count, int64_t* bin_pos, double* bin_sum,
                                     double* out, void* workspace, size_t workspace_bytes,
                                     gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K18 hub ablation (additive to ABI 32: new symbols only, no struct touched): the degree ranking
 *     and nested edge ablation of src/analysis/hub_ablation.py:56-71 (build_edge_index_ablated)  */
/* ------------------------------------------------------------------------ */
/*
 * gnn_hub_rank: for edge_index[2, E] (contiguous int64, ids in [0, N), TRUSTED: the caller checks them)
 *   deg[v]         = #{e : src[e] = v} + #{e : dst[e] = v}   (a self loop counts 2, duplicates each time)
 *   order[N]       = the nodes by (deg descending, node id ascending);   rank[N] = its inverse
 *   edge_rank[e]   = min(rank[src[e]], rank[dst[e]])
 *   removed_cum[r] = #{e : edge_rank[e] <= r}
 * all int32 (deg is an unsigned count: deg <= 2 E < 2^32).  Integer atomics, one stable radix sort:
 * bitwise reproducible.  torch.topk leaves the order of equal degrees unspecified; this tie rule (lower
 * id first) gives topk's set exactly when deg[order[h-1]] > deg[order[h]].  num_edges = 0 launches
 * nothing and writes nothing.  INVALID_ARG before any launch: a negative size, num_edges or num_nodes
 * >= INT32_MAX, edges without nodes, a null buffer; WORKSPACE for a missing or short one.
 *
 * gnn_hub_ablate: out[2, kept] = the columns e of edge_index with edge_rank[e] >= num_hubs, in input
 * order: the graph without every edge that touches one of order[0 .. num_hubs).  `kept` is the caller's
 * E - removed_cum[num_hubs - 1], as gnn_edge_drop's E - drop_count: no host synchronisation,
 * capturable; a column whose output position is not below `kept` is not written.  num_edges = 0,
 * num_hubs = 0 (the caller keeps edge_index itself) and kept = 0 launch nothing.  INVALID_ARG before any
 * launch: negative num_edges, num_edges >= INT32_MAX, num_hubs outside [0, INT32_MAX) (the ranking's
 * num_nodes, below INT32_MAX, is not an argument here: the caller holds num_hubs <= num_nodes), kept
 * outside [0, num_edges], a null buffer; WORKSPACE for a missing or short one.
 */
gnn_status gnn_hub_rank_workspace_size(int64_t num_nodes, int64_t num_edges, size_t* bytes);
gnn_status gnn_hub_rank(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes, int32_t* deg,
                        int32_t* order, int32_t* rank, int32_t* edge_rank, int32_t* removed_cum,
                        void* workspace, size_t workspace_bytes, gnn_stream_t stream);
gnn_status gnn_hub_ablate_workspace_size(int64_t num_edges, size_t* bytes);
gnn_status gnn_hub_ablate(const int64_t* edge_index, int64_t num_edges, const int32_t* edge_rank,
                          int64_t num_hubs, int64_t kept, int64_t* out, void* workspace,
                          size_t workspace_bytes, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K19 run reports (additive to ABI 32: new symbols only, no struct touched): what the tools of the
 *     reference's "Analysis" section need beyond K14 / K17 — src/analysis/workload_curves.py,
 *     eval_by_time.py and evaluate_ensemble.py (calibration_plots.py reads K17's bins)          */
/* ------------------------------------------------------------------------ */
#define GNN_REPORT_MAX_SEGMENTS 2048     /* groups of gnn_segment_threshold_counts (one block's LDS histogram) */
/* further bits of the device status word (GNN_RANK_STATUS_* above; the caller zeroes and reads it) */
#define GNN_REPORT_STATUS_K 8            /* a ks[j] is below 1: its outputs are 0, 0, NaN */
#define GNN_JOIN_STATUS_DUPLICATE 16     /* an id occurs twice in base_ids or in other_ids */
#define GNN_JOIN_STATUS_NEGATIVE 32      /* an id is negative */
#define GNN_JOIN_STATUS_MISMATCH 64      /* the two arrays do not hold the same set of ids */
/* gnn_ensemble_pair's mode */
#define GNN_ENSEMBLE_PROB 0
#define GNN_ENSEMBLE_LOGIT 1

/*
 * gnn_rank_hits_at: for a ONE-segment plan (order, seg_ptr; m = seg_ptr[1] stays on the device),
 * positive[n] indexed by element and ks[num_k] (DEVICE int64, each >= 1):
 *   k_eff[j] = min(ks[j], m);   hits[j] = positives among plan positions 0 .. k_eff[j] - 1 (int64);
 *   precision[j] = (double)hits[j] / (double)k_eff[j], NaN when m = 0.
 * One inclusive scan of the labels in plan order and one gather: integer counts and one IEEE division,
 * bitwise reproducible.  A ks[j] < 1 sets GNN_REPORT_STATUS_K and writes 0, 0, NaN.  num_k = 0 launches
 * nothing.  INVALID_ARG before any launch: negative n or num_k, n >= INT32_MAX, num_segments != 1, a null
 * buffer; WORKSPACE for a missing or short one.
 */
gnn_status gnn_rank_hits_at_workspace_size(int64_t n, size_t* bytes);
gnn_status gnn_rank_hits_at(const int32_t* order, const int32_t* seg_ptr, const uint8_t* positive, int64_t n,
                            int64_t num_segments, const int64_t* ks, int64_t num_k, int64_t* k_eff,
                            int64_t* hits, double* precision, int32_t* status, void* workspace,
                            size_t workspace_bytes, gnn_stream_t stream);

/*
 * gnn_segment_threshold_counts: one pass over scores[n] (f32), positive[n], include[n] (NULL = all) and
 * segment[n] (int32 in [0, S)), no sort and no plan: counts[S, 4] (int64) = per segment the TP, FP and FN
 * of (double)score >= thr and the number of included elements.  An included element whose segment is
 * outside [0, S) sets GNN_RANK_STATUS_SEGMENT and is skipped.  Integer sums (LDS atomics per block, the
 * blocks' rows added in block order): the same bits whatever the order.  thr must be a float32 value, as
 * for gnn_threshold_calibration.  S = 0 launches nothing.  INVALID_ARG before any launch: a negative
 * size, S > GNN_REPORT_MAX_SEGMENTS, thr not a float32 value, a null buffer; WORKSPACE for a missing or
 * short one.
 */
gnn_status gnn_segment_threshold_counts_workspace_size(int64_t n, int64_t num_segments, size_t* bytes);
gnn_status gnn_segment_threshold_counts(const float* scores, const uint8_t* positive, const uint8_t* include,
                                        const int32_t* segment, int64_t n, int64_t num_segments, double thr,
                                        int64_t* counts, int32_t* status, void* workspace,
                                        size_t workspace_bytes, gnn_stream_t stream);

/*
 * gnn_id_join: perm[n] (int32) with other_ids[perm[i]] == base_ids[i] for two DEVICE int64 arrays that
 * hold the same n distinct non-negative ids.  Two stable radix sorts of (id, position) pairs over all 64
 * key bits, an element-wise comparison of the sorted keys and a scatter.  Status bits:
 * GNN_JOIN_STATUS_DUPLICATE (adjacent equal sorted keys in either array), GNN_JOIN_STATUS_NEGATIVE,
 * GNN_JOIN_STATUS_MISMATCH (sorted keys differ); perm is unspecified (but written inside [0, n)) when any
 * is set.  n = 0 launches nothing.  INVALID_ARG before any launch: negative n, n >= INT32_MAX, a null
 * buffer; WORKSPACE for a missing or short one.
 */
gnn_status gnn_id_join_workspace_size(int64_t n, size_t* bytes);
gnn_status gnn_id_join(const int64_t* base_ids, const int64_t* other_ids, int64_t n, int32_t* perm,
                       int32_t* status, void* workspace, size_t workspace_bytes, gnn_stream_t stream);

/*
 * gnn_ensemble_pair: out[i] (f32) from x = a[perm_a[i]] (a[i] when perm_a is NULL) and y = b[i], both f32:
 *   GNN_ENSEMBLE_PROB   0.5f * (x + y) in f32 (numpy's 0.5 * (pa + pb) on f32 scores, bit for bit);
 *   GNN_ENSEMBLE_LOGIT  x, y clipped in f32 to [(float)1e-6, (float)(1 - 1e-6)], then in f64, every
 *                       operation rounded once: r = sqrt(x y), q = sqrt((1 - x)(1 - y)),
 *                       out = (float)(r / (r + q)) — the closed form of sigma((logit x + logit y) / 2).
 * A NaN input sets GNN_RANK_STATUS_NAN, a perm_a[i] outside [0, n) GNN_RANK_STATUS_INDEX; both write NaN.
 * Element-wise: no workspace.  n = 0 launches nothing.  INVALID_ARG before any launch: negative n,
 * n >= INT32_MAX, another mode, a null buffer.
 */
gnn_status gnn_ensemble_pair(const float* a, const float* b, const int32_t* perm_a, int64_t n, int32_t mode,
                             float* out, int32_t* status, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K20 feature-only baseline (additive to ABI 32: new symbols only, no struct touched): the logistic
 *     regression of src/train_baselines.py and the isotonic / Platt calibrators of
 *     src/utils/calibrate.py:32-47, as logreg.py and calibrate.py define them                       */
/* ------------------------------------------------------------------------ */
#define GNN_LOGREG_MAX_D 255             /* feature columns of a fit (D + 1 <= 256: the H tiles of one block) */
#define GNN_LOGREG_ROWS 128              /* listed rows per block: one partial (F, g, H) slab each */
#define GNN_LOGREG_REDUCE_UNROLL 4       /* slabs a reduce thread loads per step (the adds stay one chain) */
#define GNN_ISOTONIC_CHUNK 128           /* tie groups per independent PAVA chunk */
/* bits of the K20 calls' device status word (the caller zeroes and reads it) */
#define GNN_BASELINE_STATUS_ROW 1        /* a listed row is outside [0, num_rows): it was skipped */
#define GNN_BASELINE_STATUS_NAN 2        /* gnn_isotonic_apply: a query is NaN (NaN is written) */

/*
 * Common to the three row-list calls: x[num_rows, D] f32 with row stride ld >= D, rows[n] (int32; NULL =
 * the rows 0 .. n-1) the selected rows in order, 1 <= D <= GNN_LOGREG_MAX_D.  mu[D], sd[D] (f64; both
 * NULL = raw columns) standardise on the fly: z_ij = ((double)x_ij - mu_j) / sd_j, never stored.  n = 0
 * launches nothing.  INVALID_ARG before any launch: a negative size, D outside its range, ld < D, n or
 * num_rows >= INT32_MAX, a null buffer, one of mu / sd without the other; WORKSPACE for a missing or short
 * one.  A listed row outside [0, num_rows) sets GNN_BASELINE_STATUS_ROW and is skipped.
 *
 * gnn_column_moments: mu_j = sum x_ij / n, var_j = sum (x_ij - mu_j)^2 / n (two passes, f64),
 * sd_j = sqrt(var_j), 1 where var_j == 0.  Sums in row order inside a block of GNN_LOGREG_ROWS rows, the
 * blocks in block order: bitwise reproducible.
 */
gnn_status gnn_column_moments_workspace_size(int64_t n, int64_t D, size_t* bytes);
gnn_status gnn_column_moments(const float* x, int64_t ld, int64_t num_rows, const int32_t* rows, int64_t n,
                              int64_t D, double* mu, double* sd, int32_t* status, void* workspace,
                              size_t workspace_bytes, gnn_stream_t stream);

/*
 * gnn_logreg_eval: at theta[D + 1] = (w, b) (f64, device), with t_i = z_i.w + b, y[num_rows] bytes indexed
 * by row (non-zero = positive) and s_i = w1 for a positive row, w0 otherwise:
 *   F = C sum_i s_i (softplus(t_i) - y_i t_i) + 1/2 |w|^2                       (the intercept is free)
 *   g[D + 1] = C A^T r + (w, 0),  r_i = s_i (sigma(t_i) - y_i)                  A = [Z | 1]
 *   H[D + 1, D + 1] = C A^T S A + diag(1, .., 1, 0),  S_i = s_i sigma(t_i) sigma(-t_i)
 * all f64, sigma and softplus through exp(-|t|).  value_only != 0 writes F alone (g, H may be NULL).
 * Each block of GNN_LOGREG_ROWS rows writes one partial slab (one triangle of H); a second launch adds
 * the slabs in order and mirrors the triangle: H is bitwise symmetric and two runs give the same bits.
 * No atomics on floats.  Also INVALID_ARG: C not positive and finite, a negative or non-finite weight.
 */
gnn_status gnn_logreg_eval_workspace_size(int64_t n, int64_t D, size_t* bytes);
gnn_status gnn_logreg_eval(const float* x, int64_t ld, int64_t num_rows, const int32_t* rows, int64_t n,
                           int64_t D, const uint8_t* y, const double* mu, const double* sd, double w0,
                           double w1, double C, const double* theta, int32_t value_only, double* F, double* g,
                           double* H, int32_t* status, void* workspace, size_t workspace_bytes,
                           gnn_stream_t stream);

/* gnn_logreg_predict: p[k] = sigma(z_k.w + b) of listed row k, as f64 (p64) and / or f32 (p32); a row
 * outside x writes NaN.  No workspace. */
gnn_status gnn_logreg_predict(const float* x, int64_t ld, int64_t num_rows, const int32_t* rows, int64_t n,
                              int64_t D, const double* mu, const double* sd, const double* theta, double* p64,
                              float* p32, int32_t* status, gnn_stream_t stream);

/*
 * gnn_isotonic_fit: the isotonic regression (sklearn's IsotonicRegression(out_of_bounds="clip") thresholds)
 * of positive[] on scores[] over the included elements of a ONE-segment rank plan of those scores
 * (gnn_rank_plan_build: order, flags, seg_ptr).  The points are the plan's tie groups in ascending score
 * order, each with integers P (positives) and W (elements); PAVA pools adjacent blocks a, b while
 * P_a W_b >= P_b W_a (int64), a block's value is the f64 division P / W, and of the interior points only
 * those whose value differs from a neighbour's are kept.  xs[K], ys[K] (f64, room for n each) and *K
 * (device int64) are written; no included element gives K = 0.  Integer-exact: the same bits whatever the
 * chunking (GNN_ISOTONIC_CHUNK groups per independent chunk, then pairwise merges that pool outward from
 * each seam).  n = 0 launches nothing.  INVALID_ARG before any launch: negative n, n >= INT32_MAX,
 * num_segments != 1, a null buffer; WORKSPACE for a missing or short one.
 */
gnn_status gnn_isotonic_fit_workspace_size(int64_t n, size_t* bytes);
gnn_status gnn_isotonic_fit(const float* scores, const int32_t* order, const uint8_t* flags,
                            const int32_t* seg_ptr, const uint8_t* positive, int64_t n, int64_t num_segments,
                            double* xs, double* ys, int64_t* K, void* workspace, size_t workspace_bytes,
                            gnn_stream_t stream);

/*
 * gnn_isotonic_apply: out[i] for the f32 queries, in f64 with every operation rounded once (scipy's linear
 * interp1d as sklearn calls it): x clipped to [xs[0], xs[K-1]], j = clip(lower_bound(xs, x), 1, K - 1),
 * slope = (ys[j] - ys[j-1]) / (xs[j] - xs[j-1]), out = slope (x - xs[j-1]) + ys[j-1]; K = 1 gives ys[0],
 * K = 0 the query itself.  out64 and / or out32 = (float)out.  A NaN query sets GNN_BASELINE_STATUS_NAN
 * and writes NaN.  INVALID_ARG before any launch: negative n, n >= INT32_MAX, a null buffer.
 */
gnn_status gnn_isotonic_apply(const double* xs, const double* ys, const int64_t* K, const float* queries,
                              int64_t n, double* out64, float* out32, int32_t* status, gnn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K21 epoch loop (additive to ABI 32: new symbols and new structs only): the best-state and
 *     early-stopping bookkeeping of train_gnn.main's epoch loop (src/train_gnn.py:371-392) on the
 *     device, so that an epoch needs no host decision (epoch_loop.py)                               */
/* ------------------------------------------------------------------------ */
#define GNN_EPOCH_MAX_TENSORS 64         /* (src, dst, bytes) entries of one call's table */
#define GNN_EPOCH_CHUNK_BYTES 16384      /* bytes of one entry that one block copies */

typedef struct {
  const void* src;  /* device; 4-byte aligned */
  void* dst;        /* device; 4-byte aligned; must not overlap any src */
  int64_t bytes;    /* >= 0, a multiple of 4; 0: the entry is skipped (src, dst may be NULL) */
} gnn_epoch_tensor;

typedef struct {
  int32_t num_tensors; /* 0 .. GNN_EPOCH_MAX_TENSORS */
  int32_t reserved;
  gnn_epoch_tensor tensors[GNN_EPOCH_MAX_TENSORS];
} gnn_epoch_table;

/* the device state block (32 bytes); a run starts from {0, 0, 0, 0, 0, 0, -1.0} */
typedef struct {
  int32_t epoch;      /* epochs run so far */
  int32_t bad;        /* epochs since the best one */
  int32_t best_epoch; /* 1-based; 0: none yet */
  int32_t stop_epoch; /* the epoch the run ended on; 0: still running */
  int32_t status;     /* the AP status bits that ended the run (the host raises for them) */
  int32_t reserved;
  double best_val;
} gnn_epoch_state;

/*
 * gnn_epoch_keep_best: one epoch's bookkeeping.  ap (f64), ap_status (int32) and loss (f32) are device
 * scalars read when the launch runs, table a HOST struct read at the call (its pointers travel in the
 * kernel arguments: a captured launch replays them).  With s = *state:
 *
 *   if s.stop_epoch != 0 or s.epoch >= max_epochs: return      (frozen: nothing is read or written)
 *   e = s.epoch + 1;  s.epoch = e;  loss_log[e-1] = loss;  ap_log[e-1] = ap
 *   if ap_status != 0:  s.status |= ap_status;  s.stop_epoch = e
 *   else:
 *     if ap > s.best_val:  s.best_val = ap;  s.bad = 0;  s.best_epoch = e;  every src -> dst, byte for byte
 *     else:                s.bad += 1                       (a tie or a NaN ap is "not better")
 *     if s.bad >= patience or e == max_epochs:  s.stop_epoch = e
 *
 * Two launches, so that every block acts on the state as it was before the call: the copy first — each
 * block takes the decision itself from *state, *ap and *ap_status, none of which that launch writes —
 * then one thread updates the state and the logs.  The copy moves 16 bytes per lane where src and dst are
 * both 16-byte aligned (the last bytes % 16 as 4-byte words) and 4-byte words otherwise, one block per
 * GNN_EPOCH_CHUNK_BYTES of an entry; a table without bytes launches no copy.  loss_log[max_epochs] f32,
 * ap_log[max_epochs] f64.  INVALID_ARG before any launch: a null pointer, num_tensors outside its range,
 * an entry with negative bytes, bytes % 4 != 0, or with bytes > 0 a null or misaligned src / dst,
 * patience < 0, max_epochs < 1.
 */
gnn_status gnn_epoch_keep_best(const double* ap, const int32_t* ap_status, const float* loss,
                               const gnn_epoch_table* table, int32_t patience, int32_t max_epochs,
                               gnn_epoch_state* state, float* loss_log, double* ap_log, gnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNMP_H_ */
