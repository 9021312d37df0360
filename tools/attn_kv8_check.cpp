// Isolated conformance check of the fp8 K/V panel kernels (vlog_amd/csrc/attn_dec.hip, engine option cross_kv_fp8):
// launch_cross_attn_fp8 and the device quantiser launch_kv8_quant alone, no engine, no model.
//
// Per environment (H = 2 heads, 3 slots, T = 1500 whose last 64-key tile holds 28 keys, and T = 1472 = 23 x 64):
// bf16 K / V panels are drawn with the forcing generators of tools/attn_check_ref.h, quantised on the DEVICE
// (codes and exponent bytes between guards) and dequantised on the HOST (e4m3 value x 2^e: exactly bf16 values, which
// is asserted).  Every case then runs twice with the same arguments, on the fp8 launcher and on the bf16 launcher over
// the dequantised panels, and must meet two criteria:
//   (a) the fp8 launcher's output, captured probabilities and split partials pass the f64 criterion of attn_check_ref.h
//       with the bf16 family's per-element tolerances, the dequantised panels being the inputs (they are exact bf16
//       values, so the kernels' rounding steps are the same count);
//   (b) output, split partials (m, l, o) and captured probabilities are memcmp-equal between the two launchers.
//       Required for cross_tf (its arithmetic after LDS is the bf16 kernel's); for the three VALU kernels the program
//       prints per family how many cases are identical and the largest difference in bf16 ulps, and (a) still binds.
// The quantiser shares one exponent per 64-value key row, so a row that carries a profile level (stairs / under /
// edges: up to ~300 nats) keeps that level to 4 significant bits and flushes its noise: the staircases turn into steps
// of zero or more than the deferred-rescale threshold mixed with steps below it, the maxima in the ragged tile (first /
// last) stay.  The reference sees exactly these values.
// Outputs, probabilities and split scratch are prefilled with the position-dependent sentinel; bytes outside the write
// set must be unchanged; all buffers sit between 0xFF guards.
//
// Usage: attn_kv8_check cross_tf|cross_group|cross_capture|cross_dec|all [-v]
// One line per non-passing case, then `family <name>: ok|FAIL`.  Exit 0 ok, 1 mismatch, 2 HIP error (at once).
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <cstdio>
#include <string>

#include "../vlog_amd/csrc/attn.h"
#include "attn_check_ref.h"

using namespace acr;

static bool g_verbose = false;

#define CK(x)                                                                         \
  do {                                                                                \
    hipError_t e__ = (x);                                                             \
    if (e__ != hipSuccess) {                                                          \
      std::printf("HIP error: %s: %s\n", #x, hipGetErrorString(e__));                 \
      std::fflush(stdout);                                                            \
      _exit(2);                                                                       \
    }                                                                                 \
  } while (0)

template <class F>
static void launch(const char* what, F f) {
  try {
    f();
  } catch (const std::exception& e) {
    std::printf("HIP error: %s: %s\n", what, e.what());
    std::fflush(stdout);
    _exit(2);
  }
  CK(hipDeviceSynchronize());
}
template <class F>
static bool throws(F f) {
  try {
    f();
  } catch (const std::exception&) {
    return true;
  }
  CK(hipDeviceSynchronize());
  return false;
}

constexpr size_t GUARD = 512;
struct DBuf {
  uint8_t* raw = nullptr;
  size_t bytes = 0;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  ~DBuf() { if (raw) (void)hipFree(raw); }
  void alloc(size_t n) {
    if (raw) CK(hipFree(raw));
    bytes = n;
    CK(hipMalloc((void**)&raw, n + 2 * GUARD));
    CK(hipMemset(raw, 0xFF, n + 2 * GUARD));
  }
  void put(const void* src, size_t n) {
    alloc(n);
    CK(hipMemcpy(raw + GUARD, src, n, hipMemcpyHostToDevice));
  }
  template <class T> void put(const std::vector<T>& v) { put(v.data(), v.size() * sizeof(T)); }
  void sentinel_fill(size_t n) {
    alloc(n);
    std::vector<uint8_t> s(n);
    fill_sentinel(s.data(), n);
    CK(hipMemcpy(raw + GUARD, s.data(), n, hipMemcpyHostToDevice));
  }
  template <class T> T* p() const { return (T*)(raw + GUARD); }
  std::vector<uint8_t> get() const {
    std::vector<uint8_t> v(bytes);
    if (bytes) CK(hipMemcpy(v.data(), raw + GUARD, bytes, hipMemcpyDeviceToHost));
    return v;
  }
  size_t guards_bad() const {
    std::vector<uint8_t> g(2 * GUARD);
    CK(hipMemcpy(g.data(), raw, GUARD, hipMemcpyDeviceToHost));
    CK(hipMemcpy(g.data() + GUARD, raw + GUARD + bytes, GUARD, hipMemcpyDeviceToHost));
    return guard_damage(g.data(), 2 * GUARD, 0xFF);
  }
};

struct Fam {
  std::string name;
  bool need_identity = false;            // criterion (b) binds (cross_tf)
  int fails = 0, cases = 0, ident = 0, ident_cases = 0;
  long long max_ulp = 0;
  double worst = 0;
  std::string worst_case;
  void result(const std::string& cs, bool ok, double ratio, const std::string& detail = "") {
    ++cases;
    if (ratio > worst) { worst = ratio; worst_case = cs; }
    if (!ok) ++fails;
    if (!ok || g_verbose)
      std::printf("  %s %s %s ratio %.3f %s\n", ok ? "ok  " : "FAIL", name.c_str(), cs.c_str(), ratio, detail.c_str());
  }
  void identity(const std::string& cs, bool same, long long ulp) {
    ++ident_cases;
    ident += same;
    max_ulp = std::max(max_ulp, ulp);
    if (!same || g_verbose)
      std::printf("  %s %s %s fp8 launcher %s the bf16 launcher on the dequantised panels (largest difference %lld bf16 ulp)\n",
                  same ? "ok  " : (need_identity ? "FAIL" : "note"), name.c_str(), cs.c_str(), same ? "identical to" : "NOT identical to", ulp);
    if (!same && need_identity) { ++fails; ++cases; }
  }
  void guards(const std::string& cs, std::initializer_list<const DBuf*> bufs) {
    size_t bad = 0;
    for (const DBuf* b : bufs)
      if (b->raw) bad += b->guards_bad();
    if (bad) result(cs + " guards", false, INFINITY, std::to_string(bad) + " guard bytes changed");
  }
  int finish() {
    std::printf("family %s: bit identity with the bf16 launcher in %d of %d cases (largest difference %lld bf16 ulp)\n", name.c_str(),
                ident, ident_cases, max_ulp);
    std::printf("family %s: %s (%d cases, worst error/tolerance %.3f at %s)\n", name.c_str(), fails ? "FAIL" : "ok", cases, worst,
                worst_case.c_str());
    std::fflush(stdout);
    return fails ? 1 : 0;
  }
};

static const double THR_TF = CROSS_TF_RESCALE_THR;

static std::vector<int> bounds_of(int T, int n) {
  std::vector<int> b;
  const int ch = (T + n - 1) / n;
  for (int s = 0; s < n; ++s) b.push_back(s * ch);
  return b;
}

// ==================================================================================================================
// Panels: drawn bf16 -> device quantiser -> host dequantiser -> the bf16 panels both criteria are stated on
struct Env {
  int H = 0, NS = 0, T = 0;
  std::vector<uint16_t> Kq, Vq;          // dequantised, bf16 bits [slot][H][T][64]
  std::vector<double> Kd, Vd;
  DBuf dKq, dVq, dK8, dV8, dKe, dVe;
  void make(Fam& F, int H_, int NS_, int T_, uint64_t seed) {
    H = H_; NS = NS_; T = T_;
    const size_t rows = (size_t)NS * H * T, n = rows * HD;
    std::vector<uint16_t> K(n), V(n);
    Rng g(seed);
    const std::vector<int> bounds = bounds_of(T, 12);
    for (int s = 0; s < NS; ++s)
      for (int h = 0; h < H; ++h)
        for (int t = 0; t < T; ++t) {
          const size_t o = (((size_t)s * H + h) * T + t) * HD;
          gen_key_row(g, t, T, THR_TF, bounds, HD, &K[o]);
          gen_val_row(g, HD, s == 0, &V[o]);
        }
    DBuf dK, dV;
    dK.put(K); dV.put(V);
    dK8.sentinel_fill(n); dV8.sentinel_fill(n); dKe.sentinel_fill(rows); dVe.sentinel_fill(rows);
    launch("launch_kv8_quant", [&] {
      launch_kv8_quant(dK.p<bf16>(), (long long)rows, (long long)rows, (long long)rows, 0, dK8.p<unsigned char>(),
                       dKe.p<unsigned char>(), nullptr, nullptr);
      launch_kv8_quant(dV.p<bf16>(), (long long)rows, (long long)rows, (long long)rows, 0, dV8.p<unsigned char>(),
                       dVe.p<unsigned char>(), nullptr, nullptr);
    });
    F.guards("quantiser", {&dK, &dV, &dK8, &dV8, &dKe, &dVe});
    Kq.resize(n); Vq.resize(n); Kd.resize(n); Vd.resize(n);
    size_t inexact = 0;
    double worst_rel = 0;
    auto deq = [&](const DBuf& codes, const DBuf& exps, const std::vector<uint16_t>& src, std::vector<uint16_t>& qb, std::vector<double>& qd) {
      const auto c = codes.get(), e = exps.get();
      for (size_t r = 0; r < rows; ++r) {
        double amax = 0;
        for (int i = 0; i < HD; ++i) amax = std::max(amax, std::fabs((double)b2f(src[r * HD + i])));
        for (int i = 0; i < HD; ++i) {
          const double v = std::ldexp(e4m3(c[r * HD + i]), (int)e[r] - 127);
          const float f = (float)v;
          inexact += (double)f != v || b2f(f2b(f)) != f;
          qb[r * HD + i] = f2b(f);
          qd[r * HD + i] = v;
          // the quantiser's own bound: the scaled amax lies in (224, 448], so half a step of its binade is at most
          // 16 / 256 (or 8 / 224) of amax
          if (amax > 0) worst_rel = std::max(worst_rel, std::fabs(v - (double)b2f(src[r * HD + i])) / amax);
        }
      }
    };
    deq(dK8, dKe, K, Kq, Kd);
    deq(dV8, dVe, V, Vq, Vd);
    F.result("dequantised panels are exact bf16 values", inexact == 0, inexact ? INFINITY : 0, std::to_string(inexact) + " values");
    F.result("quantisation error <= amax / 16 per value", worst_rel <= 1.0 / 16.0, worst_rel * 16.0);
    dKq.put(Kq); dVq.put(Vq);
  }
  CrossKv8 kv8() const {
    CrossKv8 kv;
    kv.k = dK8.p<unsigned char>(); kv.v = dV8.p<unsigned char>(); kv.kexp = dKe.p<unsigned char>(); kv.vexp = dVe.p<unsigned char>();
    return kv;
  }
};

struct Cfg {
  int rows = 1, group = 1, plan_rows = 0;
  int done = 0;                          // 0 no table, 1 a third of the hypotheses (finished rows inside live groups), 2 + the whole first group
  bool probs = false;
  int tf = 0, mfma = 0;
  int gen_shift = 0;
};
struct Res {
  std::vector<uint8_t> out, probs, pm, pl, po;
};

static int cross_splits(const Cfg& c, int H, int T, bool& use_tf) {
  const int plan_rows = std::max(c.plan_rows, c.rows);
  const bool mf_tf = c.tf && c.group >= 16, mf_dec = !c.tf && c.mfma && c.group >= 2 && c.group <= 32 && !c.probs;
  use_tf = (mf_tf || mf_dec) && c.rows % c.group == 0;
  if (use_tf) {
    if (!mf_dec) return 1;
    const int nqt = (c.group + 127) / 128, ntt = (T + 63) / 64, pb = plan_rows / c.group * H * nqt;
    return std::max(1, std::min(std::min(16, ntt), (256 + pb - 1) / pb));
  }
  if (c.probs) return 1;
  int rg = 1;
  for (int k = 8; k >= 1; --k)
    if (c.group % k == 0 && c.rows % k == 0) { rg = k; break; }
  const int pb = plan_rows / rg * H;
  const int s = ((rg == 1 ? 10240 : 2048) + pb - 1) / pb;
  return std::max(1, std::min(s, std::min(16, (T + 127) / 128)));
}

static long long bf16_ulps(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
  long long w = 0;
  auto key = [](uint16_t u) { return (u & 0x8000) ? -(long long)(u & 0x7FFF) : (long long)u; };
  for (size_t i = 0; i + 1 < a.size(); i += 2) {
    uint16_t x, y;
    std::memcpy(&x, &a[i], 2);
    std::memcpy(&y, &b[i], 2);
    w = std::max(w, std::llabs(key(x) - key(y)));
  }
  return w;
}

// One case: both launchers with the same arguments, criterion (a) on the fp8 launcher, criterion (b) between them
static void run_case(Fam& F, Env& E, const Cfg& c, const std::string& cs) {
  const int H = E.H, T = E.T, d = H * HD, rows = c.rows, group = c.group;
  const int n_align = 2;                 // head 0 -> slot 0, head 1 not captured; slot 1 belongs to no head: never written
  std::vector<int> head_map(H, -1);
  head_map[0] = 0;
  std::vector<int> row_hyp(rows), hyp_slot(rows), done(rows, 0);
  for (int r = 0; r < rows; ++r) row_hyp[r] = rows - 1 - r;                              // non-identity, groups contiguous
  for (int hy = 0; hy < rows; ++hy) {
    hyp_slot[hy] = ((rows - 1 - hy) / group + 1) % E.NS;                                 // first window in slot 1: never slot 0 alone
    if (c.done >= 1) done[hy] = hy % 3 == 1;
  }
  if (c.done >= 2)
    for (int r = 0; r < std::min(group, rows); ++r) done[row_hyp[r]] = 1;
  auto row_slot = [&](int r) { return hyp_slot[row_hyp[r - r % group]]; };
  auto row_done = [&](int r) { return c.done && done[row_hyp[r]]; };
  std::vector<uint16_t> q((size_t)rows * d);
  {
    Rng g(2000 + rows * 31 + group + c.gen_shift);
    for (int r = 0; r < rows; ++r)
      for (int h = 0; h < H; ++h) gen_query(g, mixed_gen(r + h + c.gen_shift), HD, 8.0, &q[(size_t)r * d + h * HD]);
  }
  bool use_tf = false;
  const int splits = cross_splits(c, H, T, use_tf);
  DBuf dq, drh, dhs, ddone, dhm;
  dq.put(q); drh.put(row_hyp); dhs.put(hyp_slot); ddone.put(done); dhm.put(head_map);
  const int OROWS = rows + 2;
  const size_t np = (size_t)rows * H * 16;
  CrossFuse fz;
  fz.tf = c.tf; fz.mfma = c.mfma;
  Res res[2];
  for (int f8 = 0; f8 < 2; ++f8) {
    DBuf dout, dprobs, dpm, dpl, dpo;
    dpm.sentinel_fill(np * 4); dpl.sentinel_fill(np * 4); dpo.sentinel_fill(np * HD * 4);
    dout.sentinel_fill((size_t)OROWS * d * 2);
    if (c.probs) dprobs.sentinel_fill((size_t)OROWS * n_align * T * 4);
    float* pr = c.probs ? dprobs.p<float>() : nullptr;
    const int* hm = c.probs ? dhm.p<int>() : nullptr;
    const int* dn = c.done ? ddone.p<int>() : nullptr;
    if (f8)
      launch("launch_cross_attn_fp8", [&] {
        launch_cross_attn_fp8(dq.p<bf16>(), d, E.kv8(), T, dhs.p<int>(), drh.p<int>(), dn, dout.p<bf16>(), d, rows, H, group,
                              dpm.p<float>(), dpl.p<float>(), dpo.p<float>(), pr, hm, n_align, c.plan_rows, 0, fz, nullptr, nullptr,
                              nullptr, nullptr);
      });
    else
      launch("launch_cross_attn", [&] {
        launch_cross_attn(dq.p<bf16>(), d, E.dKq.p<bf16>(), E.dVq.p<bf16>(), T, dhs.p<int>(), drh.p<int>(), dn, dout.p<bf16>(), d, rows,
                          H, group, dpm.p<float>(), dpl.p<float>(), dpo.p<float>(), pr, hm, n_align, c.plan_rows, 0, fz, nullptr,
                          nullptr, nullptr, nullptr);
      });
    res[f8].out = dout.get();
    if (c.probs) res[f8].probs = dprobs.get();
    res[f8].pm = dpm.get(); res[f8].pl = dpl.get(); res[f8].po = dpo.get();
    F.guards(cs + (f8 ? " fp8" : " bf16"), {&dq, &drh, &dhs, &ddone, &dhm, &dout, &dprobs, &dpm, &dpl, &dpo, &E.dK8, &E.dV8, &E.dKe, &E.dVe,
                                            &E.dKq, &E.dVq});
  }
  const Res& r8 = res[1];
  // (b)
  const bool same = r8.out == res[0].out && r8.probs == res[0].probs && r8.pm == res[0].pm && r8.pl == res[0].pl && r8.po == res[0].po;
  F.identity(cs, same, bf16_ulps(r8.out, res[0].out));
  // the split scratch outside the write set
  {
    Image im_m(np), im_o(np * HD);
    if (splits > 1)
      for (int r = 0; r < rows; ++r) {
        if (row_done(r)) continue;
        for (int h = 0; h < H; ++h)
          for (int s2 = 0; s2 < splits; ++s2) {
            const size_t pi = ((size_t)r * H + h) * splits + s2;
            im_m.tol[pi] = INFINITY;
            for (int x = 0; x < HD; ++x) im_o.tol[pi * HD + x] = INFINITY;
          }
      }
    const size_t bad = compare<float>(im_m, r8.pm).sentinel_bad + compare<float>(im_m, r8.pl).sentinel_bad + compare<float>(im_o, r8.po).sentinel_bad;
    F.result(cs + " split scratch outside the write set", bad == 0, bad ? INFINITY : 0, std::to_string(bad) + " bytes changed");
  }
  // (a)
  std::vector<Att> ref((size_t)rows * H);
  std::vector<long long> all(T);
  for (int t = 0; t < T; ++t) all[t] = t;
  auto qd = [&](int r, int h, double* o) { for (int e = 0; e < HD; ++e) o[e] = b2f(q[(size_t)r * d + h * HD + e]); };
  parallel_for(rows * H, [&](int i) {
    const int r = i / H, h = i % H;
    double qv[HD];
    qd(r, h, qv);
    const size_t o = ((size_t)row_slot(r) * H + h) * T * HD;
    attend(qv, HD, scale_log2(), &E.Kd[o], HD, &E.Vd[o], HD, HD, all.data(), T, HD, ref[i]);
  });
  Image im((size_t)OROWS * d);
  for (int r = 0; r < rows; ++r) {
    if (row_done(r)) continue;
    for (int h = 0; h < H; ++h) {
      const Att& a = ref[(size_t)r * H + h];
      for (int e = 0; e < HD; ++e) {
        const size_t i = (size_t)r * d + h * HD + e;
        im.ref[i] = a.o[e];
        im.tol[i] = tol_out(a.o[e], a.A[e], a.ds, a.n, use_tf, a.vmax[e]);
      }
    }
  }
  const Cmp co = compare<uint16_t>(im, r8.out);
  F.result(cs + " splits " + std::to_string(splits) + (use_tf ? " mfma" : " valu"), co.ok(), co.w.ratio, co.str());
  if (c.probs) {
    Image ip((size_t)OROWS * n_align * T);
    double worst_sum = 0;
    for (int r = 0; r < rows; ++r) {
      if (row_done(r)) continue;
      for (int h = 0; h < H; ++h) {
        if (head_map[h] < 0) continue;
        const Att& a = ref[(size_t)r * H + h];
        double sum = 0;
        for (int t = 0; t < T; ++t) {
          const size_t i = ((size_t)r * n_align + head_map[h]) * T + t;
          ip.ref[i] = a.p[t];
          ip.tol[i] = tol_prob(a.p[t], a.ds, T);
          float f;
          std::memcpy(&f, &r8.probs[i * 4], 4);
          sum += f;
        }
        worst_sum = std::max(worst_sum, std::fabs(sum - 1.0) / (T * U24));
      }
    }
    const Cmp cp = compare<float>(ip, r8.probs);
    F.result(cs + " probs", cp.ok(), cp.w.ratio, cp.str());
    F.result(cs + " probs row sums", worst_sum <= 1.0, worst_sum);
  }
  if (splits > 1) {
    // the unnormalised f32 partials through the LSE form, as tools/attn_check does for the bf16 family
    std::vector<Worst> ws(rows * H);
    parallel_for(rows * H, [&](int i) {
      const int r = i / H, h = i % H;
      if (row_done(r)) return;
      double qv[HD];
      qd(r, h, qv);
      const size_t o = ((size_t)row_slot(r) * H + h) * T * HD;
      for (int s = 0; s < splits; ++s) {
        int b, e;
        if (use_tf) { const int ntt = (T + 63) / 64; b = s * ntt / splits * 64; e = std::min(T, (s + 1) * ntt / splits * 64); }
        else { const int ch = (T + splits - 1) / splits; b = s * ch; e = std::min(T, b + ch); }
        Att a;
        attend(qv, HD, scale_log2(), &E.Kd[o], HD, &E.Vd[o], HD, HD, all.data() + b, e - b, HD, a);
        const size_t pi = ((size_t)r * H + h) * splits + s;
        float m, l;
        std::memcpy(&m, &r8.pm[pi * 4], 4);
        std::memcpy(&l, &r8.pl[pi * 4], 4);
        ws[i].see(std::fabs((double)m + std::log2((double)l) - a.lse), tol_lse(a.lse, a.ds, a.n), (long long)pi);
        const double slack = 2 * a.ds + 2 * U24 * std::fabs(a.smax);
        if (!(m <= a.smax + slack && m >= a.smax - (use_tf ? THR_TF : 0.0) - slack)) ws[i].see(INFINITY, 1, (long long)pi);
        for (int x = 0; x < HD; ++x) {
          float ov;
          std::memcpy(&ov, &r8.po[(pi * HD + x) * 4], 4);
          const double tol = tol_out(0.0, a.A[x], a.ds, a.n, use_tf, a.vmax[x]);
          ws[i].see(std::fabs((double)ov / (double)l - a.o[x]), tol, (long long)(pi * HD + x));
        }
      }
    });
    Worst w;
    for (auto& x : ws) if (x.at >= 0) w.merge(x);
    F.result(cs + " partials (LSE form)", w.ok(), w.ratio, "worst at record " + std::to_string(w.at));
  }
}

static const int TS[2] = {1500, 1472};

static int fam_cross_tf() {
  Fam F{"cross_tf"};
  F.need_identity = true;
  int k = 0;
  for (int T : TS) {
    Env E;
    E.make(F, 2, 3, T, 21 + T);
    const std::string ts = "T " + std::to_string(T) + " ";
    // decode: beam groups of 2, 5, 32 rows in two windows; 16 key splits, and one split (a plan of many windows)
    for (int group : {2, 5, 32})
      for (int one = 0; one < 2; ++one)
        for (int dn : {0, 1, 2}) {
          if (dn && (group == 2 || (one && dn == 2))) continue;
          Cfg c;
          c.group = group; c.rows = 2 * group; c.mfma = 1; c.plan_rows = one ? 256 * group : 0; c.done = dn; c.gen_shift = k++;
          run_case(F, E, c, ts + "decode group " + std::to_string(group) + (one ? " plan 256 windows" : "") +
                                (dn == 2 ? " done+group" : dn ? " done" : ""));
        }
    // teacher-forced: 16, 129 (two row tiles) and 220 rows, with a captured head (two passes, exact max) and without
    for (int group : {16, 129, 220})
      for (int pb = 0; pb < 2; ++pb)
        for (int dn = 0; dn < 2; ++dn) {
          if (dn && group != 129) continue;
          Cfg c;
          c.group = group; c.rows = group == 16 ? 32 : group; c.tf = 1; c.probs = pb; c.done = dn; c.gen_shift = k++;
          run_case(F, E, c, ts + "tf group " + std::to_string(group) + (pb ? " capture" : " no capture") + (dn ? " done" : ""));
        }
    if (T == 1500) {
      const bool th = throws([&] {
        CrossFuse fz;
        fz.tf = 1;
        launch_cross_attn_fp8(E.dKq.p<bf16>(), 128, E.kv8(), T, nullptr, E.dKq.p<int>(), nullptr, E.dKq.p<bf16>(), 128, 16, 2, 16, nullptr,
                              nullptr, nullptr, nullptr, nullptr, 0, 16, 0, fz, nullptr, nullptr, nullptr, nullptr);
      });
      F.result("fp8 panels without a slot table refused", th, th ? 0 : INFINITY);
    }
  }
  return F.finish();
}

static int fam_cross_group() {
  Fam F{"cross_group"};
  int k = 0;
  for (int T : TS) {
    Env E;
    E.make(F, 2, 3, T, 31 + T);
    const std::string ts = "T " + std::to_string(T) + " ";
    struct RG { int rows, group; };
    // RG 1, 2, 5, 8 (cross_attn_group_kernel<RG>): 12 key splits, and one split
    for (const RG rg : {RG{3, 1}, RG{4, 2}, RG{10, 5}, RG{16, 8}})
      for (int one = 0; one < 2; ++one)
        for (int dn : {0, 1, 2}) {
          if (dn && one) continue;
          Cfg c;
          c.rows = rg.rows; c.group = rg.group; c.plan_rows = one ? 12000 * rg.group : 0; c.done = dn; c.gen_shift = k++;
          run_case(F, E, c, ts + "rows " + std::to_string(rg.rows) + " group " + std::to_string(rg.group) + (one ? " one split" : "") +
                                (dn == 2 ? " done+group" : dn ? " done" : ""));
        }
  }
  return F.finish();
}

static int fam_cross_capture() {
  Fam F{"cross_capture"};
  int k = 0;
  for (int T : TS) {
    Env E;
    E.make(F, 2, 3, T, 41 + T);
    const std::string ts = "T " + std::to_string(T) + " ";
    struct RG { int rows, group; };
    // cross_capture_kernel<8>: groups of 5, 8 and 9 rows (9: two blocks per group, the second with one row)
    for (const RG rg : {RG{10, 5}, RG{16, 8}, RG{18, 9}})
      for (int dn : {0, 1, 2}) {
        Cfg c;
        c.rows = rg.rows; c.group = rg.group; c.probs = true; c.done = dn; c.gen_shift = k++;
        run_case(F, E, c, ts + "rows " + std::to_string(rg.rows) + " group " + std::to_string(rg.group) + (dn == 2 ? " done+group" : dn ? " done" : ""));
      }
  }
  return F.finish();
}

static int fam_cross_dec() {
  Fam F{"cross_dec"};
  int k = 0;
  for (int T : TS) {
    Env E;
    E.make(F, 2, 3, T, 51 + T);
    const std::string ts = "T " + std::to_string(T) + " ";
    // dec_attn_kernel<cross>: capture with one row per window
    for (int rows : {1, 7})
      for (int dn : {0, 1}) {
        if (dn && rows == 1) continue;
        Cfg c;
        c.rows = rows; c.group = 1; c.probs = true; c.done = dn; c.gen_shift = k++;
        run_case(F, E, c, ts + "rows " + std::to_string(rows) + (dn ? " done" : ""));
      }
  }
  return F.finish();
}

int main(int argc, char** argv) {
  std::string which = argc > 1 ? argv[1] : "all";
  for (int i = 2; i < argc; ++i)
    if (std::string(argv[i]) == "-v") g_verbose = true;
  int dev = 0;
  CK(hipGetDeviceCount(&dev));
  if (dev < 1) { std::printf("HIP error: no device\n"); return 2; }
  CK(hipSetDevice(0));
  struct { const char* name; int (*f)(); } fams[] = {
      {"cross_tf", fam_cross_tf}, {"cross_group", fam_cross_group}, {"cross_capture", fam_cross_capture}, {"cross_dec", fam_cross_dec}};
  int rc = 0;
  bool any = false;
  for (auto& f : fams)
    if (which == "all" || which == f.name) { any = true; rc |= f.f(); }
  if (!any) { std::printf("unknown family %s\n", which.c_str()); return 1; }
  return rc;
}
