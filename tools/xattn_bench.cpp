// Microbenchmark of the factored cross-attention kernel (vlog_amd/csrc/attn_xenc.hip) on the bench shape:
// large-v3, W windows, one row per window (greedy decode step), all windows live, bf16 and fp8 (e4m3) cross
// memory.  Times the kernel per launch with HIP events for several key-split counts and ablations (bit 0: no S
// MFMAs, bit 1: no cross-wave sum, bit 2: no U phase, bit 4: no E loads), and reports the algorithmic
// encoder-output bytes per second.  Usage: xattn_bench [W] [splits...]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../vlog_amd/csrc/attn.h"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

int main(int argc, char** argv) {
  const int W = argc > 1 ? atoi(argv[1]) : 150, H = 20, T = 1500, d = 1280, iters = 20;
  std::vector<int> split_list;
  for (int i = 2; i < argc; ++i) split_list.push_back(atoi(argv[i]));
  if (split_list.empty()) split_list = {3};
  bf16 *enc, *qp, *pu;
  float *pml, *scale;
  int *slot, *rh;
  CK(hipMalloc(&enc, (size_t)W * ((T + 31) / 32) * 32 * d * 2));   // tile-blocked slots (T padded)
  CK(hipMalloc(&qp, (size_t)W * H * d * 2));
  CK(hipMalloc(&pu, (size_t)16 * W * H * d * 2));
  CK(hipMalloc(&pml, (size_t)16 * W * H * 2 * 4));
  CK(hipMalloc(&scale, (size_t)W * T * 4));
  CK(hipMalloc(&slot, W * 4));
  CK(hipMalloc(&rh, W * 4));
  std::vector<int> id(W);
  for (int i = 0; i < W; ++i) id[i] = i;
  std::vector<float> one((size_t)W * T, 0.01f);
  CK(hipMemcpy(slot, id.data(), W * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(rh, id.data(), W * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(scale, one.data(), one.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemset(enc, 0x3c, (size_t)W * ((T + 31) / 32) * 32 * d * 2));   // bf16 ~0.0117 / e4m3 0x3c = 1.5: finite scores
  CK(hipMemset(qp, 0x3c, (size_t)W * H * d * 2));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  // XB_ABL="0,7" restricts the ablation list, XB_F8=0|1 the cross-memory form (default: all).  Sustained
  // runs lower the clock: the first configuration measured reads fastest, so compare in alternating order.
  std::vector<int> abls = {0, 1, 2, 4, 7, 16, 23};
  if (const char* e = getenv("XB_ABL")) {
    abls.clear();
    for (const char* p = e; *p;) {
      abls.push_back(atoi(p));
      while (*p && *p != ',') ++p;
      if (*p) ++p;
    }
  }
  const int f8_only = getenv("XB_F8") ? atoi(getenv("XB_F8")) : -1;
  // XB_SNAKE=1: consecutive launches walk the items in opposite orders (Infinity Cache reuse between launches)
  const int snake = getenv("XB_SNAKE") ? atoi(getenv("XB_SNAKE")) : 0;
  int launch_no = 0;
  const int keep = getenv("XB_KEEP") ? atoi(getenv("XB_KEEP")) : 0;   // windows loaded with the default policy
  for (int f8 = 0; f8 < 2; ++f8) {
    if (f8_only >= 0 && f8 != f8_only) continue;
    const double bytes = (double)W * T * d * (f8 ? 1 : 2);
    for (int abl : abls) {
      xattn_set_ablation(abl);
      for (int splits : split_list) {
        auto run = [&] {
          launch_xattn(qp, enc, f8 ? scale : nullptr, slot, rh, nullptr, W, W, 1, H, T, d, splits, snake ? (launch_no++ & 1) : 0, keep, pu, pml,
                       nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr);
        };
        for (int i = 0; i < 3; ++i) run();
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < iters; ++i) run();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        const double us = 1000.0 * ms / iters;
        printf("%s%s abl %2d splits %2d  %8.2f us  %7.1f GB/s (encoder output)\n", f8 ? "fp8 " : "bf16", snake ? " snake" : "", abl, splits, us,
               bytes / (us * 1e-6) / 1e9);
      }
    }
  }
  return 0;
}
