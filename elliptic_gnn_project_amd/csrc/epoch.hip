// K21 — the epoch loop's bookkeeping on the device (train_gnn.main's loop, src/train_gnn.py:371-392):
// "new best? keep the state : bad += 1; stop?" as one call per epoch, so that a block of epochs can be
// enqueued, or replayed from a HIP graph, without a host decision between them (epoch_loop.py).
//
// One decision per call, taken from the state as it was before the call, without a grid-wide hand-off:
//
//   epoch_copy_kernel    every block evaluates  stop_epoch == 0 && epoch < max_epochs && ap_status == 0 &&
//                        ap > best_val  itself — words this launch never writes — and, when it holds, copies
//                        its chunk of one table entry.
//   epoch_decide_kernel  one thread applies the rule to the state block and appends to the two logs.  It
//                        runs after the copy in stream order, so no block of the copy can see its writes.
//
// (A "last block" ticket that would fold the two launches costs more than the second launch on this
// part: DESIGN §8.2.)  The table travels in the kernel arguments (64 entries of 24 bytes and the entries'
// first blocks), so a captured call replays with the pointers it was captured with.
//
// The copy treats every entry as bytes (f32 parameters, f32 BN statistics, the int64 num_batches_tracked:
// all multiples of 4): 16 bytes per lane where src and dst are both 16-byte aligned, with the last
// bytes % 16 as 4-byte words, and 4-byte words otherwise.  Plain vector loads and stores.
#include "common.hpp"

namespace gnnmp {
namespace {

constexpr int kTB = 256;
constexpr int64_t kChunk = GNN_EPOCH_CHUNK_BYTES;
static_assert(kChunk % (kTB * 16) == 0, "a chunk is whole 16-byte rounds of the block");

struct CopyArgs {
  int32_t num_tensors;
  int32_t first_block[GNN_EPOCH_MAX_TENSORS + 1];  // entry t owns the blocks [first_block[t], first_block[t+1])
  gnn_epoch_tensor tensors[GNN_EPOCH_MAX_TENSORS];
};

__global__ __launch_bounds__(kTB) void epoch_copy_kernel(CopyArgs a, const double* __restrict__ ap,
                                                         const int32_t* __restrict__ ap_status,
                                                         const gnn_epoch_state* __restrict__ state,
                                                         int32_t max_epochs) {
  // the decision, from words nobody writes during this launch (a NaN ap compares false)
  if (state->stop_epoch != 0 || state->epoch >= max_epochs || *ap_status != 0 || !(*ap > state->best_val)) return;
  const int32_t b = (int32_t)blockIdx.x;
  int t = 0;
  while (t + 1 < a.num_tensors && a.first_block[t + 1] <= b) ++t;  // (uniform: scalar loads of the arguments)
  const gnn_epoch_tensor e = a.tensors[t];
  const int64_t lo = (int64_t)(b - a.first_block[t]) * kChunk;
  const int64_t hi = lo + kChunk < e.bytes ? lo + kChunk : e.bytes;  // lo < e.bytes: the host counted the blocks
  const char* __restrict__ src = static_cast<const char*>(e.src);
  char* __restrict__ dst = static_cast<char*>(e.dst);
  int64_t word0 = lo;  // the 4-byte path starts here
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const int64_t hi16 = lo + (hi - lo) / 16 * 16;  // (lo is a multiple of 16)
    for (int64_t o = lo + (int64_t)threadIdx.x * 16; o < hi16; o += (int64_t)kTB * 16)
      *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(src + o);
    word0 = hi16;
  }
  for (int64_t o = word0 + (int64_t)threadIdx.x * 4; o < hi; o += (int64_t)kTB * 4)
    *reinterpret_cast<uint32_t*>(dst + o) = *reinterpret_cast<const uint32_t*>(src + o);
}

__global__ void epoch_decide_kernel(const double* __restrict__ ap, const int32_t* __restrict__ ap_status,
                                    const float* __restrict__ loss, int32_t patience, int32_t max_epochs,
                                    gnn_epoch_state* __restrict__ state, float* __restrict__ loss_log,
                                    double* __restrict__ ap_log) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  gnn_epoch_state s = *state;
  if (s.stop_epoch != 0 || s.epoch >= max_epochs) return;  // frozen
  const int32_t e = s.epoch + 1;
  const double v = *ap;
  const int32_t st = *ap_status;
  s.epoch = e;
  loss_log[e - 1] = *loss;
  ap_log[e - 1] = v;
  if (st != 0) {
    s.status |= st;
    s.stop_epoch = e;
  } else {
    if (v > s.best_val) {
      s.best_val = v;
      s.bad = 0;
      s.best_epoch = e;
    } else {
      s.bad += 1;
    }
    if (s.bad >= patience || e == max_epochs) s.stop_epoch = e;
  }
  *state = s;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" gnn_status gnn_epoch_keep_best(const double* ap, const int32_t* ap_status, const float* loss,
                                          const gnn_epoch_table* table, int32_t patience, int32_t max_epochs,
                                          gnn_epoch_state* state, float* loss_log, double* ap_log,
                                          gnn_stream_t stream) {
  const char* fn = "gnn_epoch_keep_best";
  if (!ap || !ap_status || !loss || !table || !state || !loss_log || !ap_log)
    return fail(GNN_ERR_INVALID_ARG, fn, "null pointer");
  if (patience < 0 || max_epochs < 1) return fail(GNN_ERR_INVALID_ARG, fn, "patience < 0 or max_epochs < 1");
  if (table->num_tensors < 0 || table->num_tensors > GNN_EPOCH_MAX_TENSORS)
    return fail(GNN_ERR_INVALID_ARG, fn, "num_tensors outside [0, GNN_EPOCH_MAX_TENSORS]");
  CopyArgs a{};
  int64_t blocks = 0;
  for (int t = 0; t < table->num_tensors; ++t) {
    const gnn_epoch_tensor& e = table->tensors[t];
    if (e.bytes < 0 || e.bytes % 4 != 0) return fail(GNN_ERR_INVALID_ARG, fn, "an entry's bytes are negative or no multiple of 4");
    if (e.bytes > 0 && (!e.src || !e.dst || (((uintptr_t)e.src | (uintptr_t)e.dst) & 3) != 0))
      return fail(GNN_ERR_INVALID_ARG, fn, "an entry's src / dst is null or not 4-byte aligned");
    a.tensors[t] = e;
    a.first_block[t] = (int32_t)blocks;
    blocks += ceil_div(e.bytes, kChunk);
    if (blocks >= INT32_MAX) return fail(GNN_ERR_INVALID_ARG, fn, "the table is too large for one launch");
  }
  a.num_tensors = table->num_tensors;
  for (int t = table->num_tensors; t <= GNN_EPOCH_MAX_TENSORS; ++t) a.first_block[t] = (int32_t)blocks;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (blocks > 0) {
    hipLaunchKernelGGL(epoch_copy_kernel, dim3((unsigned)blocks), dim3(kTB), 0, s, a, ap, ap_status, state, max_epochs);
    GNN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(epoch_decide_kernel, dim3(1), dim3(1), 0, s, ap, ap_status, loss, patience, max_epochs, state,
                     loss_log, ap_log);
  GNN_LAUNCH_CHECK();
  return GNN_OK;
}
