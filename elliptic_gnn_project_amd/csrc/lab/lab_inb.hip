// Kernel lab (not part of the library): the half-pair NT with its B fragments formed in the
// kernel's prologue from the Linear weights (gemm_nt_h2_kernel INB) against the B-image prep launch
// + the image form, at the SAGE layer-1 shape.  Checks C and z bit for bit, then times the two
// alternating (hip events around `reps` back-to-back launches each).
//   make -C elliptic_gnn_project_amd/csrc labinb;  ./lab_inb [M] [reps] [rounds]
#define GNNMP_LAB 1
#include "../gemm_planes.hip"
#include "../gemm_ws.hip"

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

constexpr int EPIF = WS_BIAS | WS_RELU | WS_DROP | WS_PROJ;

int main(int argc, char** argv) {
  const int64_t M = argc > 1 ? std::atoll(argv[1]) : 203769;
  const int reps = argc > 2 ? std::atoi(argv[2]) : 20;
  const int rounds = argc > 3 ? std::atoi(argv[3]) : 15;
  const int64_t F = 166, LD = 336, NR = 128;
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
  std::vector<float> hw1(NR * F), hw2(NR * F), hb(NR), hp(4 * NR);
  {
    std::mt19937 g(5);
    std::normal_distribution<float> d(0.f, 1.f);
    for (auto& v : hw1) v = d(g) * 0.08f;
    for (auto& v : hw2) v = d(g) * 0.08f;
    for (auto& v : hb) v = d(g) * 0.1f;
    for (auto& v : hp) v = d(g);
  }
  float *w1 = up(hw1), *w2 = up(hw2), *bias = up(hb), *proj = up(hp);
  float *c[2], *z[2];
  for (int i = 0; i < 2; ++i) {
    CK(hipMalloc(&c[i], M * NR * 4));
    CK(hipMalloc(&z[i], M * 4 * 4));
  }
  NTArgs n{};
  n.M = M; n.Nc = NR; n.k1 = F; n.k2 = F; n.w1 = w1; n.w2 = w2; n.ldw1 = F; n.ldw2 = F; n.ldc = NR;
  n.bias = bias; n.relu = 1; n.dropout = 1; n.keep_thresh = (uint32_t)(0.5 * 16777216.0); n.drop_scale = 2.f;
  n.seed = 1234; n.proj = proj; n.nproj = 4; n.ldz = 4; n.wvec2 = 1;
  n.ap = imh; n.ap_ld = LD; n.ap_col2 = 168; n.ap_ps = M * LD; n.ap_h2 = 1;
  NTArgs na = n, nb = n;
  na.c = c[0]; na.z = z[0];
  nb.c = c[1]; nb.z = z[1];
  uint4* bh;
  CK(hipMalloc(&bh, 21 * 3 * 256 * 16 + 128 * 4));
  float* cs = reinterpret_cast<float*>(bh + 21 * 3 * 256);
  const int ntiles = (int)ceil_div(M, 32);
  const int grid = std::min(ntiles, 256);
  auto image = [&]() {
    ws_prep_h2_kernel<<<WS_PREP_GRID, WS_PREP_THREADS>>>(h2_prep_of(na, bh));
    gemm_nt_h2_kernel<21, EPIF, 0, 0><<<grid, 256>>>(na, bh, cs, ntiles);
  };
  auto inb = [&]() { gemm_nt_h2_kernel<21, EPIF, 0, 1><<<grid, 256>>>(nb, nullptr, nullptr, ntiles); };
  image();
  inb();
  CK(hipDeviceSynchronize());
  {
    std::vector<float> a(M * NR), b(M * NR), za(M * 4), zb(M * 4);
    CK(hipMemcpy(a.data(), c[0], a.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(b.data(), c[1], b.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(za.data(), z[0], za.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(zb.data(), z[1], zb.size() * 4, hipMemcpyDeviceToHost));
    const bool same = !std::memcmp(a.data(), b.data(), a.size() * 4) && !std::memcmp(za.data(), zb.data(), za.size() * 4);
    std::printf("C and z bit-identical: %s\n", same ? "yes" : "NO");
    if (!same) return 1;
  }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  auto timed = [&](auto&& fn) {
    CK(hipEventRecord(e0));
    for (int r = 0; r < reps; ++r) fn();
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1e3f / reps;
  };
  std::vector<float> ti, tb;
  for (int r = 0; r < rounds + 3; ++r) {
    const float a = timed(image), b = timed(inb);
    if (r >= 3) { ti.push_back(a); tb.push_back(b); }
  }
  auto rep = [](const char* name, std::vector<float> v) {
    std::sort(v.begin(), v.end());
    std::printf("%-28s median %.2f us  min %.2f  max %.2f\n", name, v[v.size() / 2], v.front(), v.back());
  };
  rep("prep launch + image NT", ti);
  rep("in-kernel B NT", tb);
  return 0;
}
