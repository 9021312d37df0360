// Microbenchmark of the projected form's beam-group cross-attention (vlog_amd/csrc/attn_dec.hip cross_tf_kernel, decode
// form) alone, on bf16 panels and on fp8 panels (engine option cross_kv_fp8): large-v3 heads, W windows of `group`
// hypotheses each (default 150 x 5 = 750 rows: config 5's decode pass), T = 1500, all rows live.  The launches walk
// NL layers' panels in turn (each layer's panels are 1.15 GB bf16 at 150 windows, far past the 256 MB Infinity Cache,
// so no launch finds its panels cached), timed per launch with HIP events; the two forms alternate (bf16, fp8, fp8,
// bf16: sustained runs lower the clock, so the first configuration measured reads fastest).  Reports the panel bytes
// per second (bf16: 2 x T x 64 x 2 B, fp8: 2 x T x 65 B per window and head) against 8 TB/s.  The fp8 panels are the
// device quantiser's output on the bf16 ones.  Usage: kv8_attn_bench [W] [group]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../vlog_amd/csrc/attn.h"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

int main(int argc, char** argv) {
  const int W = argc > 1 ? atoi(argv[1]) : 150, group = argc > 2 ? atoi(argv[2]) : 5;
  const int H = 20, T = 1500, d = H * 64, NL = 2, iters = 32, rows = W * group;
  if (W < 1 || group < 2 || group > 32) { printf("W >= 1, group 2..32 (the matrix-core decode form)\n"); return 1; }
  const size_t panel = (size_t)W * H * T * 64;                       // elements of one layer's K (or V) panels
  const size_t prow = (size_t)W * H * T;                             // their 64-value rows
  bf16 *kv, *q, *out;
  unsigned char *c8, *x8;
  float *pm, *pl, *po;
  int *rh, *hs;
  CK(hipMalloc(&kv, NL * 2 * panel * 2));
  CK(hipMalloc(&c8, NL * 2 * panel));
  CK(hipMalloc(&x8, NL * 2 * prow));
  CK(hipMalloc(&q, (size_t)rows * d * 2));
  CK(hipMalloc(&out, (size_t)rows * d * 2));
  CK(hipMalloc(&pm, (size_t)rows * H * 16 * 4));
  CK(hipMalloc(&pl, (size_t)rows * H * 16 * 4));
  CK(hipMalloc(&po, (size_t)rows * H * 16 * 64 * 4));
  CK(hipMalloc(&rh, rows * 4));
  CK(hipMalloc(&hs, rows * 4));
  std::vector<int> id(rows), slot(rows);
  for (int i = 0; i < rows; ++i) { id[i] = i; slot[i] = i / group; }
  CK(hipMemcpy(rh, id.data(), rows * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(hs, slot.data(), rows * 4, hipMemcpyHostToDevice));
  {
    // bf16 values with varied exponents and signs (a seeded byte pattern with every exponent byte forced into
    // 0x3a..0x3d / 0xba..0xbd: magnitudes 0.0005 .. 0.12), so the softmax is not flat and the rows' exponents differ
    std::vector<unsigned short> h(2 * panel);
    unsigned long long s = 0x9E3779B97F4A7C15ull;
    for (int l = 0; l < NL; ++l) {
      for (size_t i = 0; i < h.size(); ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const unsigned r = (unsigned)(s >> 33);
        h[i] = (unsigned short)((r & 0x8000) | ((0x3a + ((r >> 8) & 3)) << 8) | (r & 0xff));
      }
      CK(hipMemcpy(kv + (size_t)l * 2 * panel, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    }
    h.resize((size_t)rows * d);
    for (size_t i = 0; i < h.size(); ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const unsigned r = (unsigned)(s >> 33);
      h[i] = (unsigned short)((r & 0x8000) | 0x3f00 | (r & 0xff));   // |q| in 0.5 .. 1
    }
    CK(hipMemcpy(q, h.data(), h.size() * 2, hipMemcpyHostToDevice));
  }
  launch_kv8_quant(kv, (long long)(NL * 2 * prow), (long long)(NL * 2 * prow), (long long)(NL * 2 * prow), 0, c8, x8, nullptr, nullptr);
  CK(hipDeviceSynchronize());
  CrossFuse fz;
  fz.mfma = 1;
  int launch_no = 0;
  auto run = [&](int f8) {
    const int l = launch_no++ % NL;
    if (f8) {
      CrossKv8 p;
      p.k = c8 + (size_t)(2 * l) * panel; p.v = c8 + (size_t)(2 * l + 1) * panel;
      p.kexp = x8 + (size_t)(2 * l) * prow; p.vexp = x8 + (size_t)(2 * l + 1) * prow;
      launch_cross_attn_fp8(q, d, p, T, hs, rh, nullptr, out, d, rows, H, group, pm, pl, po, nullptr, nullptr, 0, rows, 0, fz, nullptr,
                            nullptr, nullptr, nullptr);
    } else {
      launch_cross_attn(q, d, kv + (size_t)(2 * l) * panel, kv + (size_t)(2 * l + 1) * panel, T, hs, rh, nullptr, out, d, rows, H, group,
                        pm, pl, po, nullptr, nullptr, 0, rows, 0, fz, nullptr, nullptr, nullptr, nullptr);
    }
  };
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  printf("W %d group %d rows %d H %d T %d, %d launches per figure over %d layers' panels\n", W, group, rows, H, T, iters, NL);
  for (int f8 : {0, 1, 1, 0}) {
    const double bytes = (double)W * H * T * 2 * (f8 ? 65 : 128);
    for (int i = 0; i < 4; ++i) run(f8);
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < iters; ++i) run(f8);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    const double us = 1000.0 * ms / iters, gbs = bytes / (us * 1e-6) / 1e9;
    printf("%s panels  %8.2f us per launch  %7.1f GB/s of panel bytes  %.3f of 8 TB/s\n", f8 ? "fp8 " : "bf16", us, gbs, gbs / 8000.0);
  }
  return 0;
}
