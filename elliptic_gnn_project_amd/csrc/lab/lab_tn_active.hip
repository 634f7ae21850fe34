// Kernel lab (not part of the library): the flag-driven half-pair TN (gemm_tn_h2_kernel, ACT) at the
// headline shape — M = 203,769 rows in 255 row blocks of 800, 50 consecutive row blocks fully
// flagged (the rolling train window of the step), the rest unflagged — in its first form, with the
// LAB ablations (bit 1 no MFMAs, bit 2 no staging), with deeper load rings and with the column
// split, and the slab reduce with and without the empty-slab skip.  Variants are interleaved in one
// process and timed with events (median of the rounds); every variant's slabs are compared with the
// first form's bit for bit.
//   make -C elliptic_gnn_project_amd/csrc labtnact;  ./lab_tn_active [rounds]
#define GNNMP_LAB 1
#include "../gemm_planes.hip"
#include "../gemm_ws.hip"
#include "../gemm_f32.hip"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace gnnmp {
void set_last_error(const std::string&) {}
}

#define CK(x)                                                                         \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      std::exit(1);                                                                   \
    }                                                                                 \
  } while (0)

using namespace gnnmp;

__global__ void split_h2_kernel(const float* x, int64_t n2, uint16_t* img, int64_t ps) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n2) return;
  uint32_t h, l;
  split_h2_pair(x[2 * i], x[2 * i + 1], h, l);
  reinterpret_cast<uint32_t*>(img)[i] = h;
  reinterpret_cast<uint32_t*>(img + ps)[i] = l;
}

constexpr int NRB = 255;  // row blocks
template <int LAB, int KS, int RD>
void tn(const TNArgs& a) {
  gemm_tn_h2_kernel<11, false, LAB, 8, false, KS, false, true, RD><<<KS * NRB, 512>>>(a);
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 15;
  const int64_t M = 203769, F = 166, LD = 336, NR = 128;
  const int64_t rpb = ceil_div(ceil_div(M, 32), 256) * 32;  // 800
  const int b_lo = 100, b_hi = 150;                         // the flagged row blocks
  std::vector<float> hx(M * LD, 0.f);
  {
    std::mt19937 g(1);
    std::normal_distribution<float> d(0.f, 1.f);
    for (int64_t r = 0; r < M; ++r)
      for (int c = 0; c < F; ++c) {
        hx[r * LD + c] = d(g) * 0.7f;
        hx[r * LD + 168 + c] = d(g);
      }
  }
  auto up = [](const std::vector<float>& h) {
    float* p;
    CK(hipMalloc(&p, h.size() * 4));
    CK(hipMemcpy(p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    return p;
  };
  float* xa = up(hx);
  uint16_t* imh;
  CK(hipMalloc(&imh, 2 * M * LD * 2));
  split_h2_kernel<<<(unsigned)ceil_div(M * LD / 2, 256), 256>>>(xa, M * LD / 2, imh, M * LD);
  std::vector<float> hp(4 * NR), hh(M * NR), hdz(M * 4, 0.f);
  const int64_t nf = ceil_div(M, 16);
  std::vector<uint8_t> hfl((nf + 15) / 16 * 16, 0);
  {
    std::mt19937 g(5);
    std::normal_distribution<float> d(0.f, 1.f);
    for (auto& v : hp) v = d(g);
    for (auto& v : hh) v = d(g);
    for (int64_t r = b_lo * rpb; r < std::min(M, b_hi * rpb); ++r) {
      for (int q = 0; q < 4; ++q) hdz[r * 4 + q] = d(g) * 1e-5f;
      hfl[r / 16] = 1;
    }
  }
  float *proj = up(hp), *dh = up(hh), *ddz = up(hdz);
  uint8_t* dfl;
  CK(hipMalloc(&dfl, hfl.size()));
  CK(hipMemcpy(dfl, hfl.data(), hfl.size(), hipMemcpyHostToDevice));

  const int64_t nout = NR * 332 + NR + 4 * NR + 4;
  const int64_t stride = (nout + 63) / 64 * 64;
  float *slab, *out;
  CK(hipMalloc(&slab, NRB * stride * 4));
  CK(hipMalloc(&out, stride * 4));
  TNArgs ta{};
  ta.M = M; ta.Nr = NR; ta.dz = ddz; ta.lddz = 4; ta.proj = proj; ta.nproj = 4; ta.h = dh; ta.ldh = NR; ta.hscale = 2.f;
  ta.k1 = F; ta.k2 = F; ta.slab = slab; ta.slab_stride = stride; ta.rows_per_block = rpb;
  ta.ap = imh; ta.ap_ld = LD; ta.ap_col2 = 168; ta.ap_ps = M * LD; ta.ap_h2 = 1;
  ta.dz_active = dfl;
  TNArgs te = ta;
  te.slab_empty = 1;
  const unsigned rb = (unsigned)ceil_div(ceil_div(nout, 4), kRedOut);

  struct V { const char* name; void (*f)(const TNArgs&); bool empty; std::vector<float> t; bool ablation = false; };
  std::vector<V> vs = {
      {"TN first form (1 block / row block, ring 1)", tn<0, 1, 1>, false, {}},
      {"TN first form, no MFMA", tn<1, 1, 1>, false, {}, true},
      {"TN first form, no staging", tn<2, 1, 1>, false, {}, true},
      {"TN first form, empty slabs skipped", tn<0, 1, 1>, true, {}},
      {"TN ring 2", tn<0, 1, 2>, false, {}},
      {"TN ring 3", tn<0, 1, 3>, false, {}},
      {"TN split 2 ring 2", tn<0, 2, 2>, false, {}},
      {"TN split 2 ring 3", tn<0, 2, 3>, false, {}},
      {"TN split 3 ring 3", tn<0, 3, 3>, false, {}},
      {"TN split 4 ring 1", tn<0, 4, 1>, false, {}},
      {"TN split 4 ring 2", tn<0, 4, 2>, false, {}},
      {"TN split 4 ring 3", tn<0, 4, 3>, false, {}},
      {"TN split 4 ring 4", tn<0, 4, 4>, false, {}},
      {"TN split 4 ring 3, empty slabs skipped", tn<0, 4, 3>, true, {}},
      {"TN split 3 ring 1", tn<0, 3, 1>, false, {}},
      {"TN split 3 ring 1, empty slabs skipped", tn<0, 3, 1>, true, {}},
      {"TN split 4 ring 1, empty slabs skipped", tn<0, 4, 1>, true, {}},
      {"TN split 4 ring 1, no MFMA", tn<1, 4, 1>, false, {}, true},
      {"TN split 4 ring 1, no staging", tn<2, 4, 1>, false, {}, true},
  };
  const size_t nsl = (size_t)NRB * stride;
  std::vector<float> r0(nsl), r1(nsl);
  for (size_t v = 0; v < vs.size(); ++v) {  // bits against the first form (ablations aside)
    if (vs[v].ablation) continue;
    CK(hipMemset(slab, 0, nsl * 4));
    vs[v].f(vs[v].empty ? te : ta);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy((v ? r1 : r0).data(), slab, nsl * 4, hipMemcpyDeviceToHost));
    if (!v) continue;
    size_t ndiff = 0;
    for (int b = 0; b < NRB; ++b)
      for (int64_t j = 0; j < nout; ++j) ndiff += std::memcmp(&r0[b * stride + j], &r1[b * stride + j], 4) != 0;
    std::printf("%-48s %zu slab words differ from the first form's\n", vs[v].name, ndiff);
  }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<float> tred[2];
  for (int r = 0; r < rounds + 2; ++r) {
    for (auto& v : vs) {
      CK(hipEventRecord(e0));
      v.f(v.empty ? te : ta);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 2) v.t.push_back(ms * 1e3f);
    }
    for (int em = 0; em < 2; ++em) {  // the reduce over the slabs the last variant left (empty words set)
      CK(hipEventRecord(e0));
      if (em) slab_reduce_kernel<true><<<rb, 256>>>(slab, stride, NRB, out, nout, SqOut{});
      else slab_reduce_kernel<false><<<rb, 256>>>(slab, stride, NRB, out, nout, SqOut{});
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 2) tred[em].push_back(ms * 1e3f);
    }
  }
  auto med = [](std::vector<float>& t) {
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
  };
  for (auto& v : vs) std::printf("%-48s %7.1f us (min %.1f)\n", v.name, med(v.t), v.t[0]);
  std::printf("%-48s %7.1f us (min %.1f)\n", "slab reduce, every slab read", med(tred[0]), tred[0][0]);
  std::printf("%-48s %7.1f us (min %.1f)\n", "slab reduce, empty slabs skipped", med(tred[1]), tred[1][0]);
  return 0;
}
