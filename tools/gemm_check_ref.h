// Host-only reference and comparator of tools/gemm_check (no HIP in this file: tools/gemm_check_selftest.cpp
// exercises it on the CPU).  For one (M, N, K) problem the f64 matrices acc = sum_k A W and S = sum_k |A| |W| are
// computed once; every epilogue of gemm_epi.h is then applied to them in f64, giving for each output buffer an
// `Image`: per element either (expected value, tolerance) or "not written" (the prefilled sentinel bytes must
// still be there).  Tolerances are derived per element, no fixed numbers:
//   E = (K + 8) 2^-24 (S + |bias| + |x_old|)      f32 summation error in any order (covers split-K slabs)
//   f32 outputs   |got - v| <= E + 2^-24 |v|
//   bf16 outputs  |got - v| <= 1.13 E + 2^-8 |v|  (1.13 bounds |gelu'|; 1 without the activation)
//   GELU_POS_F32  |got - v| <= 1.13 E + 2 g + 2^-24 |v|,  g = gelu_ulps 2^-24 max(1, |acc + bias|)
//   LayerNorm     2^-8 |ref| + |g_c| (N + 8) 2^-24 (|x - mean| + |mean|) rstd, against the f64 LayerNorm of the
//                 residual the device itself wrote
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace gcr {

constexpr double U24 = 1.0 / 16777216.0, U8 = 1.0 / 256.0, GELU_SLOPE = 1.13;
constexpr double GELU_ULPS_START = 8.0;   // bound assumed for the device gelu_erf (gemm_check measures it first)

// the epilogue kinds, numbered as EpiKind of gemm.h (gemm_check.cpp asserts the match)
enum { K_BF16 = 0, K_RESID_F32 = 1, K_GELU_POS_F32 = 2, K_F32 = 3, K_DEC_QKV = 4, K_CROSS_KV = 5, K_RESID_LN = 6 };

inline uint16_t f2b(float f) {            // round to nearest even, as the device's (bf16)x
  uint32_t u;
  std::memcpy(&u, &f, 4);
  u += 0x7FFF + ((u >> 16) & 1);
  return (uint16_t)(u >> 16);
}
inline float b2f(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline double gelu64(double x) { return 0.5 * x * (1.0 + std::erf(x * 0.70710678118654752440)); }

// Sentinel byte at byte offset b of an output buffer (position dependent: a shifted copy does not pass)
inline uint8_t sentinel(size_t b) { return (uint8_t)(0xA0 + b % 89); }
inline void fill_sentinel(uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) p[i] = sentinel(i);
}
// Bytes of a guard region that no longer hold `fill`; first = offset of the first one
inline size_t guard_damage(const uint8_t* g, size_t n, uint8_t fill, size_t* first = nullptr) {
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i)
    if (g[i] != fill) {
      if (!bad && first) *first = i;
      ++bad;
    }
  return bad;
}

struct ADesc {            // GemmA's row mapping
  long long ld;
  int rpb;
  long long bstride;
};
inline long long a_off(const ADesc& a, int r) {
  return a.rpb ? (long long)(r / a.rpb) * a.bstride + (long long)(r % a.rpb) * a.ld : (long long)r * a.ld;
}
inline size_t a_elems(const ADesc& a, int M, int K) { return (size_t)a_off(a, M - 1) + K; }

struct Ref {
  int M = 0, N = 0, K = 0;
  std::vector<double> acc, S;   // [M][N]
};

// acc / S of rows [0, M) (A rows through the descriptor, W rows of stride ldw), on up to 8 threads
inline void make_ref(const uint16_t* A, const ADesc& ad, const uint16_t* W, long long ldw, int M, int N, int K, Ref& o) {
  o.M = M; o.N = N; o.K = K;
  o.acc.assign((size_t)M * N, 0.0);
  o.S.assign((size_t)M * N, 0.0);
  std::vector<double> Wd((size_t)N * K);
  for (int c = 0; c < N; ++c)
    for (int k = 0; k < K; ++k) Wd[(size_t)c * K + k] = b2f(W[(size_t)c * ldw + k]);
  auto work = [&](int r0, int r1) {
    std::vector<double> a(K);
    for (int r = r0; r < r1; ++r) {
      const uint16_t* ar = A + a_off(ad, r);
      for (int k = 0; k < K; ++k) a[k] = b2f(ar[k]);
      for (int c = 0; c < N; ++c) {
        const double* w = Wd.data() + (size_t)c * K;
        double s0 = 0, s1 = 0, t0 = 0, t1 = 0;
        int k = 0;
        for (; k + 1 < K; k += 2) {
          const double p0 = a[k] * w[k], p1 = a[k + 1] * w[k + 1];
          s0 += p0; s1 += p1; t0 += std::fabs(p0); t1 += std::fabs(p1);
        }
        for (; k < K; ++k) { const double p = a[k] * w[k]; s0 += p; t0 += std::fabs(p); }
        o.acc[(size_t)r * N + c] = s0 + s1;
        o.S[(size_t)r * N + c] = t0 + t1;
      }
    }
  };
  const int nt = (int)std::max(1u, std::min(8u, std::min(std::thread::hardware_concurrency(), (unsigned)((M + 7) / 8))));
  if (nt == 1 || (double)M * N * K < 4e6) { work(0, M); return; }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t) th.emplace_back(work, (int)((long long)M * t / nt), (int)((long long)M * (t + 1) / nt));
  for (auto& t : th) t.join();
}

// One epilogue, as GemmEpi states it, with its host-side operands
struct Epi {
  int kind = K_BF16, act = 0;
  long long ldc = 0;
  int rpb = 0;
  long long bstride = 0;
  int roff = 0;
  std::vector<float> bias;             // [N] or empty
  std::vector<float> x_old;            // RESID kinds: [M][ldc] residual before the launch
  std::vector<float> pos;              // GELU_POS_F32: [rpb][ldc]
  std::vector<int> row_hyp, row_pos;   // DEC_QKV
  int d = 0, n_head = 0, head_dim = 0, n_ctx = 0, n_hyp = 0;
  int n_slots = 0, slot0 = 0;          // CROSS_KV
  std::vector<float> ln_g, ln_b;       // RESID_LN
  long long ln_ld = 0;
  double gelu_ulps = GELU_ULPS_START;
};

struct Image {
  int elem = 2;                        // bytes per element: 2 bf16, 4 f32
  std::vector<double> v, tol;
  std::vector<uint8_t> w;              // 1: written by the reference
  void init(size_t n, int e) { elem = e; v.assign(n, 0.0); tol.assign(n, 0.0); w.assign(n, 0); }
  size_t n() const { return w.size(); }
  size_t bytes() const { return w.size() * elem; }
  void set(size_t i, double val, double t) { v[i] = val; tol[i] = t; w[i] = 1; }
};
struct Expect {
  Image out, kc, vc;                   // kc / vc: DEC_QKV's caches
};

inline size_t out_elems(const Epi& e, int M, int N) {
  switch (e.kind) {
    case K_BF16: return e.rpb ? (size_t)((M + e.rpb - 1) / e.rpb) * e.bstride : (size_t)M * e.ldc;
    case K_CROSS_KV: return (size_t)(N / e.d) * e.n_slots * e.n_head * e.rpb * e.head_dim;
    default: return (size_t)M * e.ldc;
  }
}
inline size_t cache_elems(const Epi& e) { return (size_t)e.n_hyp * e.n_head * e.n_ctx * e.head_dim; }
inline int out_elem_bytes(int kind) { return (kind == K_BF16 || kind == K_DEC_QKV || kind == K_CROSS_KV) ? 2 : 4; }

// The expected image of every buffer the epilogue writes
inline void build_expect(const Ref& R, const Epi& e, Expect& x) {
  const int M = R.M, N = R.N;
  x.out.init(out_elems(e, M, N), out_elem_bytes(e.kind));
  if (e.kind == K_DEC_QKV) { x.kc.init(cache_elems(e), 2); x.vc.init(cache_elems(e), 2); }
  for (int r = 0; r < M; ++r)
    for (int c = 0; c < N; ++c) {
      const size_t i = (size_t)r * N + c;
      const double b = e.bias.empty() ? 0.0 : (double)e.bias[c];
      const bool resid = e.kind == K_RESID_F32 || e.kind == K_RESID_LN;
      const double xo = resid ? (double)e.x_old[(size_t)r * e.ldc + c] : 0.0;
      const double E = (R.K + 8) * U24 * (R.S[i] + std::fabs(b) + std::fabs(xo));
      const double u = R.acc[i] + b;
      switch (e.kind) {
        case K_BF16: {
          const double v = e.act == 1 ? gelu64(u) : u;
          const long long o = e.rpb ? (long long)(r / e.rpb) * e.bstride + (long long)(r % e.rpb + e.roff) * e.ldc
                                    : (long long)r * e.ldc;
          x.out.set((size_t)o + c, v, (e.act == 1 ? GELU_SLOPE : 1.0) * E + U8 * std::fabs(v));
          break;
        }
        case K_RESID_F32:
        case K_RESID_LN: {
          const double v = xo + u;
          x.out.set((size_t)r * e.ldc + c, v, E + U24 * std::fabs(v));
          break;
        }
        case K_GELU_POS_F32: {
          const double v = gelu64(u) + (double)e.pos[(size_t)(r % e.rpb) * e.ldc + c];
          const double g = e.gelu_ulps * U24 * std::max(1.0, std::fabs(u));
          x.out.set((size_t)r * e.ldc + c, v, GELU_SLOPE * E + 2 * g + U24 * std::fabs(v));
          break;
        }
        case K_F32: x.out.set((size_t)r * e.ldc + c, u, E + U24 * std::fabs(u)); break;
        case K_DEC_QKV: {
          const double t = E + U8 * std::fabs(u);
          if (c < e.d) {
            x.out.set((size_t)r * e.ldc + c, u, t);
          } else {
            const int c2 = c - e.d, kv = c2 >= e.d, cc = kv ? c2 - e.d : c2, h = cc / e.head_dim, e2 = cc - h * e.head_dim;
            const size_t slot = (((size_t)e.row_hyp[r] * e.n_head + h) * e.n_ctx + e.row_pos[r]) * e.head_dim + e2;
            (kv ? x.vc : x.kc).set(slot, u, t);
          }
          break;
        }
        case K_CROSS_KV: {
          const int l2 = c / e.d, cc = c - l2 * e.d, h = cc / e.head_dim, e2 = cc - h * e.head_dim;
          const int bb = r / e.rpb, t = r - bb * e.rpb;
          const size_t o = ((((size_t)l2 * e.n_slots + e.slot0 + bb) * e.n_head + h) * e.rpb + t) * e.head_dim + e2;
          x.out.set(o, u, E + U8 * std::fabs(u));
          break;
        }
      }
    }
}

// The bytes of an output buffer before the launch: the sentinel everywhere, and for the residual kinds x_old
// in the live elements
inline std::vector<uint8_t> initial_bytes(const Image& im, const Epi& e, int M, int N, bool is_out) {
  std::vector<uint8_t> b(im.bytes());
  fill_sentinel(b.data(), b.size());
  if (is_out && (e.kind == K_RESID_F32 || e.kind == K_RESID_LN))
    for (int r = 0; r < M; ++r) std::memcpy(b.data() + ((size_t)r * e.ldc) * 4, e.x_old.data() + (size_t)r * e.ldc, (size_t)N * 4);
  return b;
}

struct Report {
  size_t checked = 0, bad_val = 0, bad_sentinel = 0;
  double worst = 0;                    // max |err| / tol over the checked elements (inf for a NaN)
  std::vector<size_t> bad;             // element indices out of tolerance / with a changed sentinel byte
  bool ok() const { return bad_val == 0 && bad_sentinel == 0; }
  void merge(const Report& o) {
    checked += o.checked; bad_val += o.bad_val; bad_sentinel += o.bad_sentinel; worst = std::max(worst, o.worst);
  }
};

inline double elem_value(const void* got, int elem, size_t i) {
  if (elem == 2) return b2f(((const uint16_t*)got)[i]);
  return ((const float*)got)[i];
}

inline Report compare(const Image& im, const void* got) {
  Report rp;
  const uint8_t* gb = (const uint8_t*)got;
  for (size_t i = 0; i < im.n(); ++i) {
    if (im.w[i]) {
      const double err = std::fabs(elem_value(got, im.elem, i) - im.v[i]);
      ++rp.checked;
      double ratio = im.tol[i] > 0 ? err / im.tol[i] : (err == 0 ? 0.0 : INFINITY);
      if (!(err <= im.tol[i])) {       // also a NaN
        ++rp.bad_val;
        if (rp.bad.size() < 1000000) rp.bad.push_back(i);
        if (!(ratio == ratio)) ratio = INFINITY;
      }
      rp.worst = std::max(rp.worst, ratio);
    } else {
      bool same = true;
      for (int k = 0; k < im.elem; ++k) same &= gb[i * im.elem + k] == sentinel(i * im.elem + k);
      if (!same) {
        ++rp.bad_sentinel;
        if (rp.bad.size() < 1000000) rp.bad.push_back(i);
      }
    }
  }
  return rp;
}

// LayerNorm (eps 1e-5) of the rows x [M][ldc] in f64 -> image of ln_out [M][ln_ld] bf16
inline void build_ln_expect(const float* x, long long ldc, int M, int N, const Epi& e, Image& im) {
  im.init((size_t)M * e.ln_ld, 2);
  for (int r = 0; r < M; ++r) {
    const float* xr = x + (size_t)r * ldc;
    double mean = 0, var = 0;
    for (int c = 0; c < N; ++c) mean += xr[c];
    mean /= N;
    for (int c = 0; c < N; ++c) var += (xr[c] - mean) * (xr[c] - mean);
    var /= N;
    const double rstd = 1.0 / std::sqrt(var + 1e-5);
    for (int c = 0; c < N; ++c) {
      const double ref = (xr[c] - mean) * rstd * e.ln_g[c] + e.ln_b[c];
      const double t = U8 * std::fabs(ref) + std::fabs((double)e.ln_g[c]) * (N + 8) * U24 * (std::fabs(xr[c] - mean) + std::fabs(mean)) * rstd;
      im.set((size_t)r * e.ln_ld + c, ref, t);
    }
  }
}

}  // namespace gcr
