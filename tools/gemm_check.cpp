// Isolated conformance check of the bf16 GEMM family (tools only): every entry point of gemm.h that engine.cpp
// reaches, against the f64 reference of tools/gemm_check_ref.h (per-element tolerances derived from the
// reference, see that header), at the row / column / K edges of each route.  Every device buffer sits between two
// 4 MB canary guards (inputs' guards hold 0xFF bytes: a stray read that reaches an output makes it NaN); every
// output buffer, the K/V caches, the pad columns of ldc > N outputs and the split-K scratch are prefilled with a
// sentinel pattern, and after each launch every byte outside the reference's write set must be unchanged.  The
// bit-identity promises of gemm.h (ring column widths, LDS budgets, 4 / 8 waves, gemm_8p persistent, deferred
// combine) are asserted with memcmp.
//   usage: gemm_check skinny|tiled|ring|ring_big|oneshot|gemv|p8|big|combine|all [-v]
// Prints every case that is not a plain pass (-v: every case), one line per route and per bit-identity claim, then
// "family <name>: ok" or "family <name>: FAIL"; exit status 0 when every family is ok.
// "unsupported" = the launcher refused the shape (allowed, unless the case is marked as one engine.cpp produces).
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>
#include "../vlog_amd/csrc/gemm.h"
#include "gemm_check_ref.h"

static_assert((int)EPI_BF16 == gcr::K_BF16 && (int)EPI_RESID_F32 == gcr::K_RESID_F32 && (int)EPI_GELU_POS_F32 == gcr::K_GELU_POS_F32 &&
              (int)EPI_F32 == gcr::K_F32 && (int)EPI_DEC_QKV == gcr::K_DEC_QKV && (int)EPI_CROSS_KV == gcr::K_CROSS_KV &&
              (int)EPI_RESID_LN == gcr::K_RESID_LN, "gemm_check_ref.h numbers the epilogue kinds as gemm.h");

#define CK(x)                                                                        \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      std::fflush(stdout);                                                           \
      std::exit(2);                                                                  \
    }                                                                                \
  } while (0)

// ---------------------------------------------------------------- guarded device buffers
static const size_t GUARD = 4u << 20;
static const uint8_t FILL_IN = 0xFF, FILL_OUT = 0x5a, FILL_WS = 0x5c;
struct DBuf {
  char* base = nullptr;
  size_t bytes = 0;
  uint8_t fill = 0;
  const char* name = "";
  void* p() const { return base + GUARD; }
};
static std::vector<DBuf> g_live;
static unsigned long long* g_cnt = nullptr;

static DBuf galloc(const char* name, size_t bytes, uint8_t fill, const void* src = nullptr) {
  DBuf g;
  g.bytes = bytes; g.fill = fill; g.name = name;
  CK(hipMalloc(&g.base, bytes + 2 * GUARD));
  CK(hipMemset(g.base, fill, bytes + 2 * GUARD));
  if (src && bytes) CK(hipMemcpy(g.p(), src, bytes, hipMemcpyHostToDevice));
  g_live.push_back(g);
  return g;
}
static void free_to(size_t mark) {
  while (g_live.size() > mark) {
    CK(hipFree(g_live.back().base));
    g_live.pop_back();
  }
}

__global__ void count_ne_kernel(const uint8_t* p, size_t n, uint8_t fill, unsigned long long* cnt) {
  const size_t stride = (size_t)gridDim.x * blockDim.x * 16;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; i < n; i += stride) {
    unsigned bad = 0;
    for (int k = 0; k < 16; ++k)
      if (i + k < n) bad += p[i + k] != fill;
    if (bad) atomicAdd(cnt, (unsigned long long)bad);
  }
}
__global__ void gelu_probe_kernel(const float* x, float* y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = gelu_erf(x[i]);
}

static size_t count_ne(const void* p, size_t n, uint8_t fill) {
  if (!n) return 0;
  CK(hipMemset(g_cnt, 0, 8));
  hipLaunchKernelGGL(count_ne_kernel, dim3(1024), dim3(256), 0, 0, (const uint8_t*)p, n, fill, g_cnt);
  unsigned long long h = 0;
  CK(hipMemcpy(&h, g_cnt, 8, hipMemcpyDeviceToHost));
  return (size_t)h;
}
// bytes changed in the guards of every live buffer (on damage: which buffer, and where, through the host routine)
static size_t guards_damage() {
  CK(hipMemset(g_cnt, 0, 8));
  for (const DBuf& g : g_live) {
    hipLaunchKernelGGL(count_ne_kernel, dim3(512), dim3(256), 0, 0, (const uint8_t*)g.base, GUARD, g.fill, g_cnt);
    hipLaunchKernelGGL(count_ne_kernel, dim3(512), dim3(256), 0, 0, (const uint8_t*)g.base + GUARD + g.bytes, GUARD, g.fill, g_cnt);
  }
  unsigned long long h = 0;
  CK(hipMemcpy(&h, g_cnt, 8, hipMemcpyDeviceToHost));
  if (h) {
    std::vector<uint8_t> hb(GUARD);
    for (const DBuf& g : g_live)
      for (int side = 0; side < 2; ++side) {
        CK(hipMemcpy(hb.data(), g.base + (side ? GUARD + g.bytes : 0), GUARD, hipMemcpyDeviceToHost));
        size_t first = 0;
        const size_t bad = gcr::guard_damage(hb.data(), GUARD, g.fill, &first);
        if (bad) std::printf("    guard of %s (%s the buffer): %zu bytes changed, first at guard offset %zu\n", g.name,
                             side ? "after" : "before", bad, first);
      }
  }
  return (size_t)h;
}

// ---------------------------------------------------------------- problems and epilogues
static const size_t WSB = 64ull << 20;   // the engine's split-K scratch size
static DBuf g_ws;
static double g_gelu_ulps = gcr::GELU_ULPS_START;

struct Problem {
  int M, N, K;
  gcr::ADesc ad;
  long long ldw;
  std::vector<uint16_t> A, W;
  gcr::Ref R;
  DBuf dA, dW;
  GemmA ga() const {
    GemmA a;
    std::memset(&a, 0, sizeof(a));
    a.ptr = (const bf16*)dA.p(); a.ld = ad.ld; a.rpb = ad.rpb; a.bstride = ad.bstride;
    return a;
  }
};

// conv_T = 0: plain rows (ld = K); conv_T = T: the conv2 descriptor (K = 3d: ld = 2d, rpb = T, bstride = (2T+1) d,
// overlapping rows)
static std::unique_ptr<Problem> make_problem(int M, int N, int K, int conv_T) {
  auto P = std::make_unique<Problem>();
  P->M = M; P->N = N; P->K = K; P->ldw = K;
  if (conv_T) { const int d = K / 3; P->ad = {2LL * d, conv_T, (2LL * conv_T + 1) * d}; }
  else P->ad = {K, 0, 0};
  std::mt19937 rng(1000003u * M + 7919u * N + K + conv_T);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  P->A.resize(gcr::a_elems(P->ad, M, K));
  P->W.resize((size_t)N * K);
  for (auto& v : P->A) v = gcr::f2b(U(rng));
  const float ws = 3.f / std::sqrt((float)K);          // products of unit-ish variance whatever K
  for (auto& v : P->W) v = gcr::f2b(ws * U(rng));
  gcr::make_ref(P->A.data(), P->ad, P->W.data(), P->ldw, M, N, K, P->R);
  P->dA = galloc("A", P->A.size() * 2, FILL_IN, P->A.data());
  P->dW = galloc("W", P->W.size() * 2, FILL_IN, P->W.data());
  return P;
}

struct NamedEpi {
  std::string tag;
  gcr::Epi e;
};
enum { V_PLAIN = 0, V_GELU = 1, V_MAP = 2, V_OFFSET = 3, V_LOGITS = 4 };
static const int ROWS_PER_BATCH = 100;   // cuts through every tile height

static long long pad_ld(int N) { return N % 4 == 0 ? N + 8 : N + 3; }

// one epilogue for a problem, or false when the kind does not apply to its width
static bool make_epi(const Problem& P, int kind, int variant, NamedEpi& ne) {
  const int M = P.M, N = P.N;
  gcr::Epi e;
  std::mt19937 rng(77u * kind + variant + 31u * N + M);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  e.kind = kind;
  e.ldc = pad_ld(N);
  e.gelu_ulps = g_gelu_ulps;
  e.bias.resize(N);
  for (auto& v : e.bias) v = 0.1f * U(rng);
  switch (kind) {
    case gcr::K_BF16:
      ne.tag = variant == V_GELU ? "bf16+gelu" : variant == V_MAP ? "bf16+gelu+rowmap" : "bf16";
      if (variant != V_PLAIN) e.act = 1;
      if (variant == V_MAP) { e.rpb = ROWS_PER_BATCH; e.roff = 1; e.bstride = (ROWS_PER_BATCH + 1) * e.ldc; }
      break;
    case gcr::K_F32:
      ne.tag = "f32";
      if (variant == V_MAP) { e.bias.clear(); ne.tag = "f32 nobias"; }
      if (variant == V_LOGITS) { e.bias.clear(); e.ldc = N; ne.tag = "f32 nobias ldc=N"; }    // the logits GEMM's output
      break;
    case gcr::K_RESID_F32:
    case gcr::K_RESID_LN: {
      if (kind == gcr::K_RESID_LN && (N % 2 != 0 || N > 2048)) return false;
      const float off = variant == V_OFFSET ? 1000.f : 0.f;
      ne.tag = std::string(kind == gcr::K_RESID_LN ? "resid+ln" : "resid") + (off != 0.f ? " offset1000" : "");
      e.x_old.resize((size_t)M * e.ldc);
      for (auto& v : e.x_old) v = off + 3.f * U(rng);
      if (kind == gcr::K_RESID_LN) {
        e.ln_ld = N + 8;
        e.ln_g.resize(N);
        e.ln_b.resize(N);
        for (auto& v : e.ln_g) v = 1.f + 0.2f * U(rng);
        for (auto& v : e.ln_b) v = 0.1f * U(rng);
      }
      break;
    }
    case gcr::K_GELU_POS_F32:
      ne.tag = "gelu+pos";
      e.rpb = ROWS_PER_BATCH;
      e.pos.resize((size_t)e.rpb * e.ldc);
      for (auto& v : e.pos) v = U(rng);
      break;
    case gcr::K_DEC_QKV:
    case gcr::K_CROSS_KV: {
      if (N % 3 != 0 || (N / 3) % 4 != 0) return false;
      e.d = N / 3;
      e.head_dim = e.d % 64 == 0 ? 64 : e.d / 5;
      if (e.head_dim % 4 != 0 || e.d % e.head_dim != 0) return false;
      e.n_head = e.d / e.head_dim;
      if (kind == gcr::K_DEC_QKV) {
        ne.tag = "dec_qkv";
        e.ldc = e.d + 8;
        e.n_ctx = 23;
        e.n_hyp = (M + 22) / 23 + 1;
        while ((e.n_hyp * 23) % 7 == 0) ++e.n_hyp;
        const int total = e.n_hyp * 23;         // a non-identity permutation of the (hyp, pos) slots
        for (int r = 0; r < M; ++r) {
          const int s = (int)(((long long)r * 7 + 3) % total);
          e.row_hyp.push_back(s / 23);
          e.row_pos.push_back(s % 23);
        }
      } else {
        ne.tag = "cross_kv";
        e.ldc = 0;
        e.rpb = ROWS_PER_BATCH;
        e.n_slots = (M + e.rpb - 1) / e.rpb + 2;
        e.slot0 = 1;
      }
      break;
    }
    default: return false;
  }
  ne.e = std::move(e);
  return true;
}

static std::vector<NamedEpi> epis_for(const Problem& P, std::initializer_list<std::pair<int, int>> kinds) {
  std::vector<NamedEpi> v;
  for (auto kv : kinds) {
    NamedEpi ne;
    if (make_epi(P, kv.first, kv.second, ne)) v.push_back(std::move(ne));
  }
  return v;
}

// ---------------------------------------------------------------- one launch, checked
static bool g_verbose = false;        // -v: a line per case (by default only what is not a plain pass)
struct Row {                          // one line of a family's table: a route, or a bit-identity claim
  std::string name;
  size_t ok = 0, fail = 0, unsupported = 0;
  double worst = 0;
  std::string why;                    // the first refusal's reason / shape
};
struct Fam {
  std::string name;
  size_t cases = 0, fails = 0, unsupported = 0, refused = 0, exact = 0, exact_fails = 0;
  double worst = 0, worst_f32 = 0, worst_bf16 = 0, worst_ln = 0;
  std::vector<Row> routes, claims;
  static Row& row(std::vector<Row>& t, const std::string& name) {
    for (Row& r : t)
      if (r.name == name) return r;
    t.push_back(Row{name});
    return t.back();
  }
};
struct RunOut {
  bool supported = false, ok = false;
  std::vector<uint8_t> out, kc, vc, ln;
};
using Launch = std::function<bool(const GemmA&, const bf16*, long long, int, int, int, const GemmEpi&, float*, size_t)>;

static void print_bad(const char* what, const gcr::Image& im, const void* got, const gcr::Report& rp) {
  for (size_t j = 0; j < rp.bad.size() && j < 3; ++j) {
    const size_t i = rp.bad[j];
    if (im.w[i]) std::printf("    %s[%zu]: got %.9g, reference %.9g, tolerance %.3g\n", what, i, gcr::elem_value(got, im.elem, i), im.v[i], im.tol[i]);
    else std::printf("    %s[%zu]: a byte outside the write set changed (reads %.9g)\n", what, i, gcr::elem_value(got, im.elem, i));
  }
}

// slabs: how many [M][N] f32 slabs of the scratch the route may write (0: none); everything behind them must keep
// the scratch's fill.  defer: run with defer_combine = 1 — the outputs must stay untouched, and RunOut.out becomes
// what the host makes of the slabs (summed in split order, + bias, rounded), for a memcmp against the combined run.
static RunOut run_case(Fam& F, Problem& P, const NamedEpi& ne, const std::string& route, bool required, int slabs,
                       const Launch& fn, bool defer = false) {
  const gcr::Epi& he = ne.e;
  const int M = P.M, N = P.N, K = P.K;
  RunOut ro;
  const size_t mark = g_live.size();
  gcr::Expect ex;
  gcr::build_expect(P.R, he, ex);
  GemmEpi ge;
  std::memset(&ge, 0, sizeof(ge));
  ge.kind = he.kind; ge.act = he.act; ge.ldc = he.ldc; ge.rpb = he.rpb; ge.bstride = he.bstride; ge.roff = he.roff;
  ge.d = he.d; ge.n_head = he.n_head; ge.head_dim = he.head_dim; ge.n_ctx = he.n_ctx; ge.n_slots = he.n_slots; ge.slot0 = he.slot0;
  ge.ln_ld = he.ln_ld; ge.defer_combine = defer ? 1 : 0;
  if (!he.bias.empty()) ge.bias = (const float*)galloc("bias", he.bias.size() * 4, FILL_IN, he.bias.data()).p();
  if (!he.pos.empty()) ge.pos = (const float*)galloc("pos", he.pos.size() * 4, FILL_IN, he.pos.data()).p();
  if (!he.row_hyp.empty()) {
    ge.row_hyp = (const int*)galloc("row_hyp", he.row_hyp.size() * 4, FILL_IN, he.row_hyp.data()).p();
    ge.row_pos = (const int*)galloc("row_pos", he.row_pos.size() * 4, FILL_IN, he.row_pos.data()).p();
  }
  if (!he.ln_g.empty()) {
    ge.ln_g = (const float*)galloc("ln_g", he.ln_g.size() * 4, FILL_IN, he.ln_g.data()).p();
    ge.ln_b = (const float*)galloc("ln_b", he.ln_b.size() * 4, FILL_IN, he.ln_b.data()).p();
  }
  const std::vector<uint8_t> init_out = gcr::initial_bytes(ex.out, he, M, N, true);
  const DBuf dout = galloc("out", init_out.size(), FILL_OUT, init_out.data());
  ge.out = dout.p();
  DBuf dkc, dvc, dln;
  gcr::Image lnimg;
  if (he.kind == gcr::K_DEC_QKV) {
    const std::vector<uint8_t> ic = gcr::initial_bytes(ex.kc, he, M, N, false);
    dkc = galloc("kcache", ic.size(), FILL_OUT, ic.data());
    dvc = galloc("vcache", ic.size(), FILL_OUT, ic.data());
    ge.kcache = (bf16*)dkc.p(); ge.vcache = (bf16*)dvc.p();
  }
  if (he.kind == gcr::K_RESID_LN) {
    lnimg.init((size_t)M * he.ln_ld, 2);
    const std::vector<uint8_t> il = gcr::initial_bytes(lnimg, he, M, N, false);
    dln = galloc("ln_out", il.size(), FILL_OUT, il.data());
    ge.ln_out = (bf16*)dln.p();
  }
  CK(hipMemset(g_ws.p(), FILL_WS, WSB));
  bool launched = false;
  std::string why;
  try {
    launched = fn(P.ga(), (const bf16*)P.dW.p(), P.ldw, M, N, K, ge, (float*)g_ws.p(), WSB);
  } catch (const std::exception& e) {
    why = e.what();
  }
  CK(hipDeviceSynchronize());     // a fault ends the program here: nothing more is started on the device
  char shape[96];
  std::snprintf(shape, sizeof(shape), "M=%-4d N=%-4d K=%-4d%s", M, N, K, P.ad.rpb ? " conv2-A" : "");
  ++F.cases;
  Row& row = Fam::row(F.routes, route + (required ? "  [engine]" : ""));
  if (!launched) {
    ++F.unsupported;
    ++row.unsupported;
    if (row.why.empty()) row.why = why.empty() ? std::string("first at ") + shape : why;
    if (required) { ++F.refused; ++F.fails; }
    if (required || g_verbose) std::printf("  %-11s %-44s %-18s %s%s%s%s\n", required ? "REFUSED" : "unsupported", route.c_str(), ne.tag.c_str(), shape,
                defer ? " deferred" : "", why.empty() ? "" : "  ", why.c_str());
    free_to(mark);
    return ro;
  }
  ro.supported = true;
  gcr::Report rp;
  auto fetch = [&](const DBuf& d, std::vector<uint8_t>& h) {
    h.resize(d.bytes);
    CK(hipMemcpy(h.data(), d.p(), d.bytes, hipMemcpyDeviceToHost));
  };
  fetch(dout, ro.out);
  if (defer) {
    gcr::Image untouched = ex.out;
    std::fill(untouched.w.begin(), untouched.w.end(), 0);
    const gcr::Report r0 = gcr::compare(untouched, ro.out.data());
    rp.merge(r0);
    if (!r0.ok()) print_bad("out (deferred: must stay untouched)", untouched, ro.out.data(), r0);
    std::vector<float> part((size_t)slabs * M * N);
    CK(hipMemcpy(part.data(), g_ws.p(), part.size() * 4, hipMemcpyDeviceToHost));
    ro.out = init_out;
    for (int r = 0; r < M; ++r)
      for (int c = 0; c < N; ++c) {
        float v = 0.f;
        for (int s = 0; s < slabs; ++s) v += part[((size_t)s * M + r) * N + c];
        if (!he.bias.empty()) v = v + he.bias[c];
        const uint16_t h = gcr::f2b(v);
        std::memcpy(&ro.out[((size_t)r * he.ldc + c) * 2], &h, 2);
      }
  } else {
    const gcr::Report r0 = gcr::compare(ex.out, ro.out.data());
    rp.merge(r0);
    double& wt = ex.out.elem == 4 ? F.worst_f32 : F.worst_bf16;
    wt = std::max(wt, r0.worst);
    if (!r0.ok()) print_bad("out", ex.out, ro.out.data(), r0);
    if (he.kind == gcr::K_DEC_QKV) {
      fetch(dkc, ro.kc);
      fetch(dvc, ro.vc);
      const gcr::Report r1 = gcr::compare(ex.kc, ro.kc.data()), r2 = gcr::compare(ex.vc, ro.vc.data());
      rp.merge(r1);
      rp.merge(r2);
      F.worst_bf16 = std::max(F.worst_bf16, std::max(r1.worst, r2.worst));
      if (!r1.ok()) print_bad("kcache", ex.kc, ro.kc.data(), r1);
      if (!r2.ok()) print_bad("vcache", ex.vc, ro.vc.data(), r2);
    }
    if (he.kind == gcr::K_RESID_LN) {     // the LayerNorm judged alone: against the f64 one of the device's own residual
      fetch(dln, ro.ln);
      gcr::build_ln_expect((const float*)ro.out.data(), he.ldc, M, N, he, lnimg);
      const gcr::Report r3 = gcr::compare(lnimg, ro.ln.data());
      rp.merge(r3);
      F.worst_ln = std::max(F.worst_ln, r3.worst);
      if (!r3.ok()) print_bad("ln_out", lnimg, ro.ln.data(), r3);
    }
  }
  const size_t used = std::min(WSB, (size_t)slabs * M * N * 4);
  const size_t ws_bad = count_ne((const char*)g_ws.p() + used, WSB - used, FILL_WS);
  const size_t gd = guards_damage();
  ro.ok = rp.ok() && ws_bad == 0 && gd == 0;
  if (!ro.ok) ++F.fails;
  if (rp.worst > F.worst) F.worst = rp.worst;
  ++(ro.ok ? row.ok : row.fail);
  row.worst = std::max(row.worst, rp.worst);
  if (!ro.ok || g_verbose) std::printf("  %-11s %-44s %-18s %s%s  worst %.3f of %zu", ro.ok ? "ok" : "FAIL", route.c_str(), ne.tag.c_str(), shape,
              defer ? " deferred" : "", rp.worst, rp.checked);
  if (!ro.ok)
    std::printf("  [%zu values out of tolerance, %zu elements outside the write set changed, %zu scratch bytes behind the slabs, "
                "%zu guard bytes]", rp.bad_val, rp.bad_sentinel, ws_bad, gd);
  if (!ro.ok || g_verbose) std::printf("\n");
  free_to(mark);
  return ro;
}

static void expect_same(Fam& F, const RunOut& a, const RunOut& b, const std::string& what) {
  Row& row = Fam::row(F.claims, what.substr(0, what.find(" (")));
  if (!a.supported || !b.supported) {       // a refused run: no pair to compare (shown in the claim's line)
    ++row.unsupported;
    return;
  }
  ++F.exact;
  const bool same = a.out == b.out && a.kc == b.kc && a.vc == b.vc && a.ln == b.ln;
  if (!same) { ++F.exact_fails; ++F.fails; }
  ++(same ? row.ok : row.fail);
  if (!same || g_verbose) std::printf("  %-11s bit-identical: %s\n", same ? "ok" : "FAIL", what.c_str());
}

struct Problems {
  std::map<std::tuple<int, int, int, int>, std::unique_ptr<Problem>> m;
  Problem& get(int M, int N, int K, int conv_T = 0) {
    auto& p = m[std::make_tuple(M, N, K, conv_T)];
    if (!p) p = make_problem(M, N, K, conv_T);
    return *p;
  }
};

static const std::initializer_list<std::pair<int, int>> DEC_KINDS = {
    {gcr::K_BF16, V_GELU}, {gcr::K_RESID_F32, V_PLAIN}, {gcr::K_F32, V_PLAIN}, {gcr::K_DEC_QKV, V_PLAIN}, {gcr::K_RESID_LN, V_PLAIN}};

static Launch via_launch_gemm(bool with_ws) {
  return [with_ws](const GemmA& a, const bf16* w, long long ldw, int M, int N, int K, const GemmEpi& e, float* ws, size_t wsb) {
    launch_gemm(a, w, ldw, M, N, K, e, with_ws ? ws : nullptr, with_ws ? wsb : 0, 0);
    return true;
  };
}

// ---------------------------------------------------------------- families
// launch_gemm with a scratch, M <= 512: the skinny split-K kernel (templates switch at 16 / 32 / 64 / 128 / 160 / 256 / 320)
static void fam_skinny(Fam& F) {
  Problems Ps;
  const int Ms[] = {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 255, 256, 257, 319, 320, 321, 511, 512};
  const int Ks[] = {128, 384, 1280, 1536};
  int i = 0;
  for (int M : Ms) {
    std::vector<std::pair<int, int>> shapes = {{384, Ks[i % 4]}, {420, Ks[(i + 1) % 4]}, {1001, M > 160 ? Ks[i % 2] : Ks[(i + 2) % 4]}};
    if (M <= 33) shapes.push_back({i % 2 ? 420 : 384, 5120});
    if (M == 1 || M == 17) shapes.push_back({1001, 5120});
    ++i;
    for (auto nk : shapes) {
      const int N = nk.first, K = nk.second;
      const int s = skinny_splits(M, N, K, WSB);
      if (s <= 0) { ++F.fails; std::printf("  FAIL        skinny_splits(%d, %d, %d) = 0: launch_gemm would not take the skinny form\n", M, N, K); continue; }
      Problem& P = Ps.get(M, N, K);
      RunOut plain;
      for (const NamedEpi& ne : epis_for(P, {{gcr::K_BF16, V_PLAIN}, {gcr::K_BF16, V_MAP}, {gcr::K_RESID_F32, V_PLAIN}, {gcr::K_F32, V_PLAIN},
                                             {gcr::K_F32, V_LOGITS}, {gcr::K_DEC_QKV, V_PLAIN}, {gcr::K_RESID_LN, V_PLAIN}})) {
        if (ne.tag == "f32 nobias ldc=N" && N % 2 == 0) continue;      // the odd width only
        const bool ln = ne.e.kind == gcr::K_RESID_LN;
        const RunOut r = run_case(F, P, ne, "launch_gemm skinny splits " + std::to_string(s), true, (s > 1 || ln) ? s : 0, via_launch_gemm(true));
        if (ne.tag == "bf16") plain = r;
      }
      if (s > 1 && (M == 150 || M == 33 || M == 160 || M == 512 || M == 1)) {
        NamedEpi ne;
        make_epi(P, gcr::K_BF16, V_PLAIN, ne);
        const RunOut d = run_case(F, P, ne, "launch_gemm skinny splits " + std::to_string(s), true, s, via_launch_gemm(true), true);
        expect_same(F, plain, d, "host sum of the deferred slabs in split order vs the combined output");
      }
    }
  }
  {   // the conv2 operand descriptor (overlapping rows) through the skinny kernel's LDS-DMA row addressing
    Problem& P = Ps.get(250, 128, 384, ROWS_PER_BATCH);
    const int s = skinny_splits(250, 128, 384, WSB);
    for (const NamedEpi& ne : epis_for(P, {{gcr::K_BF16, V_MAP}, {gcr::K_RESID_F32, V_PLAIN}}))
      run_case(F, P, ne, "launch_gemm skinny splits " + std::to_string(s), true, s > 1 ? s : 0, via_launch_gemm(true));
  }
  {   // the residual offset 1000 (a one-pass variance in the fused combine would fail), at a decoder shape
    Problem& P = Ps.get(150, 384, 384);
    NamedEpi ne;
    make_epi(P, gcr::K_RESID_LN, V_OFFSET, ne);
    const int s = skinny_splits(150, 384, 384, WSB);
    run_case(F, P, ne, "launch_gemm skinny splits " + std::to_string(s), true, std::max(1, s), via_launch_gemm(true));
  }
  free_to(1);
}

// the split count of gemm.hip's run<BM, BN> (a mirror of its arithmetic, to know how much scratch it may write)
static int tiled_splits(int M, int N, int K, bool with_ws) {
  const int BM = M <= 16 ? 16 : M <= 32 ? 32 : M <= 64 ? 64 : M <= 128 ? 128 : M <= 256 ? 256 : 128, BN = M <= 256 ? 64 : 128;
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN), nk = K / 64;
  int splitk = 1;
  if (with_ws && tiles < 1024) {
    splitk = std::min(std::max(1, 1024 / tiles), std::max(1, nk / 4));
    while (splitk > 1 && (size_t)splitk * M * N * 4 > WSB) --splitk;
  }
  const int kps = (nk + splitk - 1) / splitk;
  return (nk + kps - 1) / kps;
}

// launch_gemm's tiled kernel: without a scratch (any M < 1024), and with split-K at 600 rows
static void fam_tiled(Fam& F) {
  Problems Ps;
  const std::initializer_list<std::pair<int, int>> kinds = {
      {gcr::K_BF16, V_PLAIN}, {gcr::K_BF16, V_MAP}, {gcr::K_RESID_F32, V_PLAIN}, {gcr::K_GELU_POS_F32, V_PLAIN}, {gcr::K_F32, V_PLAIN},
      {gcr::K_F32, V_MAP}, {gcr::K_F32, V_LOGITS}, {gcr::K_DEC_QKV, V_PLAIN}, {gcr::K_CROSS_KV, V_PLAIN}, {gcr::K_RESID_LN, V_PLAIN}};
  const int Ms[] = {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600};
  const int Ks[] = {64, 384, 1280};
  int i = 0;
  for (int M : Ms) {
    std::vector<std::pair<int, int>> shapes = {{384, Ks[i % 3]}, {420, Ks[(i + 1) % 3]}, {1001, Ks[(i + 2) % 3]}};
    // K = 1536 at every row count, 5120 at few rows or few columns; 1408 at 600 rows leaves a ragged last K split
    // (22 K-tiles in splits of 5)
    shapes.push_back({i % 2 ? 420 : 384, 1536});
    if (M <= 33) shapes.push_back({i % 2 ? 384 : 420, 5120});
    if (M == 600) { shapes.push_back({128, 5120}); shapes.push_back({384, 1408}); }
    ++i;
    for (auto nk : shapes) {
      Problem& P = Ps.get(M, nk.first, nk.second);
      for (int with_ws = 0; with_ws < (M == 600 ? 2 : 1); ++with_ws) {
        const int s = tiled_splits(M, nk.first, nk.second, with_ws);
        // (RESID_LN off the skinny path is the residual epilogue + launch_layernorm, which takes the model widths only:
        // a multiple of 128 here; other widths are refused by a throw after the residual was updated)
        for (const NamedEpi& ne : epis_for(P, kinds))
          run_case(F, P, ne, with_ws ? "launch_gemm tiled split-K " + std::to_string(s) : "launch_gemm tiled",
                   ne.e.kind != gcr::K_RESID_LN || nk.first % 128 == 0, s > 1 ? s : 0, via_launch_gemm(with_ws));
      }
    }
  }
  {   // > 1024 rows at an odd width (the large-tile kernels need N % 4 == 0): the 128 x 128 tiled kernel, split-K
    Problem& P = Ps.get(1030, 1001, 384);
    const int s = tiled_splits(1030, 1001, 384, true);
    for (const NamedEpi& ne : epis_for(P, {{gcr::K_F32, V_LOGITS}, {gcr::K_F32, V_PLAIN}, {gcr::K_BF16, V_MAP}, {gcr::K_RESID_F32, V_PLAIN}}))
      run_case(F, P, ne, "launch_gemm tiled split-K " + std::to_string(s), true, s > 1 ? s : 0, via_launch_gemm(true));
  }
  // the conv2 operand descriptor (overlapping rows, T = 100) with its epilogue, and the conv1 row map
  for (int M : {250, 600}) {
    Problem& P = Ps.get(M, 128, 384, ROWS_PER_BATCH);
    for (const NamedEpi& ne : epis_for(P, {{gcr::K_GELU_POS_F32, V_PLAIN}, {gcr::K_BF16, V_MAP}, {gcr::K_RESID_F32, V_PLAIN}}))
      run_case(F, P, ne, "launch_gemm tiled", true, 0, via_launch_gemm(false));
  }
  free_to(1);
}

struct RingPlan {
  int rows, cols, lds, waves;
  bool engine;          // a plan engine.cpp produces (at widths that are multiples of 128)
};
static Launch via_ring(const RingPlan& p, int kr) {
  return [p, kr](const GemmA& a, const bf16* w, long long ldw, int M, int N, int K, const GemmEpi& e, float* ws, size_t wsb) {
    return launch_dec_ring(a, w, ldw, M, N, K, e, ws, wsb, kr, 0, p.rows, p.cols, p.lds, p.waves);
  };
}
static int ring_splits(int K, int kr) {
  if (kr <= 0) kr = K <= 1280 ? K : ((K + (K + 1279) / 1280 - 1) / ((K + 1279) / 1280) + 63) / 64 * 64;
  return (K + kr - 1) / kr;
}
static std::string ring_name(const RingPlan& p, int kr) {
  char b[96];
  std::snprintf(b, sizeof(b), "dec_ring rows %d cols %d lds %d waves %d kr %d", p.rows, p.cols, p.lds, p.waves, kr);
  return b;
}
static RunOut run_ring(Fam& F, Problem& P, const NamedEpi& ne, const RingPlan& p, int kr, bool defer = false) {
  const int s = ring_splits(P.K, kr);
  const bool ln = ne.e.kind == gcr::K_RESID_LN;
  return run_case(F, P, ne, ring_name(p, kr), p.engine && P.N % 128 == 0, (s > 1 || ln) ? s : 0, via_ring(p, kr), defer);
}

// launch_dec_ring at decoder row counts (<= 160): the preset plans (row groups of 96 / 32 / 64, 32 or 64 columns; one
// group of all rows), K whole or in ranges
static void fam_ring(Fam& F) {
  Problems Ps;
  const RingPlan presets[] = {{96, 32, 0, 4, true}, {32, 32, 0, 4, true}, {64, 64, 0, 4, true}, {0, 32, 0, 4, true}};
  // the same arithmetic per row, promised bit-identical: column widths, LDS budgets, waves (against the first)
  const RingPlan same[] = {{64, 32, 144, 4, true}, {64, 64, 144, 4, true}, {64, 128, 144, 4, false}, {64, 64, 72, 4, true}, {64, 64, 144, 8, true}};
  const char* same_what[] = {"", "ring cols 64 vs 32", "ring cols 128 vs 32", "ring lds 72 vs 144", "ring 8 waves vs 4"};
  const RingPlan extra[] = {{32, 64, 0, 4, false}, {128, 128, 144, 8, false}, {160, 32, 0, 4, false}};
  const std::pair<int, int> Kkr[] = {{384, 0}, {1280, 0}, {1536, 0}, {1536, 640}, {1536, 1280}, {5120, 1280}, {5120, 640}};
  for (int N : {384, 420})
    for (auto kk : Kkr) {
      const int K = kk.first, kr = kk.second;
      Problem& P = Ps.get(150, N, K);
      for (const NamedEpi& ne : epis_for(P, DEC_KINDS)) {
        for (const RingPlan& p : presets) {
          if (p.rows == 0 && K > 1280) continue;      // engine.cpp takes that plan only for K <= 1280
          // the engine passes kr = K for K <= 1280 and 1280 above; other ranges only through decode_gemm_kr
          run_ring(F, P, ne, p, kr == 0 && K <= 1280 && p.rows > 0 ? K : kr);
        }
        RunOut first;
        for (int j = 0; j < 5; ++j) {
          const RunOut r = run_ring(F, P, ne, same[j], kr);
          if (j == 0) first = r;
          else expect_same(F, first, r, std::string(same_what[j]) + " (" + ne.tag + ", N " + std::to_string(N) + " K " + std::to_string(K) + ")");
        }
        if (K == 1536 && kr == 640)
          for (const RingPlan& p : extra) run_ring(F, P, ne, p, kr);
      }
      if (ring_splits(K, kr) > 1) {       // cq's deferred combine (decode_gemm_kr below K)
        NamedEpi ne;
        make_epi(P, gcr::K_BF16, V_PLAIN, ne);
        const RunOut a = run_ring(F, P, ne, presets[1], kr), d = run_ring(F, P, ne, presets[1], kr, true);
        expect_same(F, a, d, "host sum of the deferred ring slabs in split order vs the combined output");
      }
    }
  // other row counts: one row, a ragged second group, the largest single group
  for (int M : {1, 33, 97, 160})
    for (int N : {384, 420}) {
      Problem& P = Ps.get(M, N, 384);
      for (const NamedEpi& ne : epis_for(P, DEC_KINDS))
        for (const RingPlan& p : presets) run_ring(F, P, ne, p, p.rows > 0 ? 384 : 0);
    }
  {
    Problem& P = Ps.get(150, 384, 1536);
    NamedEpi ne;
    make_epi(P, gcr::K_RESID_LN, V_OFFSET, ne);
    run_ring(F, P, ne, presets[2], 1280);
  }
  free_to(1);
}

// launch_dec_ring on the big-rows routes: >= 161 rows in 64-row groups over the whole K; >= 512 rows on 8 waves
// (64 x 64 tiles for the d x d projections, 128 x 128 for qkv / fc1 / fc2, fc2 in K ranges of decode_gemm_big_fc2_kr)
static void fam_ring_big(Fam& F) {
  Problems Ps;
  for (int M : {161, 200, 512, 513, 1000}) {
    const bool w8 = M >= 512;
    const RingPlan sq = w8 ? RingPlan{64, 64, 144, 8, true} : RingPlan{64, 32, 144, 4, true};
    const RingPlan wide = w8 ? RingPlan{128, 128, 144, 8, true} : RingPlan{64, 64, 72, 4, true};
    struct Sh { int N, K, kr; };
    // (N, K, kr): d x d and qkv / fc1 shapes over the whole K; fc2 (K = 4d) whole and, on 8 waves, in ranges of 1280
    std::vector<Sh> shapes = {{384, 384, 384}, {420, 384, 384}, {384, 1280, 1280}, {w8 ? 128 : 384, 1536, 1536}, {128, 5120, 5120}};
    if (w8) { shapes.push_back({128, 5120, 1280}); shapes.push_back({384, 1536, 1280}); }
    for (const Sh& sh : shapes) {
      Problem& P = Ps.get(M, sh.N, sh.K);
      for (const NamedEpi& ne : epis_for(P, DEC_KINDS))
        for (const RingPlan* p : {&sq, &wide}) {
          const RunOut r = run_ring(F, P, ne, *p, sh.kr);
          if (M == 512 && p == &sq && sh.K <= 1536) {
            const RunOut r4 = run_ring(F, P, ne, RingPlan{64, 64, 144, 4, true}, sh.kr);
            expect_same(F, r4, r, "ring 8 waves vs 4 at 512 rows (" + ne.tag + ", K " + std::to_string(sh.K) + " kr " + std::to_string(sh.kr) + ")");
          }
          if (M == 200 && p == &wide && sh.K <= 1536) {
            const RunOut r144 = run_ring(F, P, ne, RingPlan{64, 64, 144, 4, true}, sh.kr);
            expect_same(F, r144, r, "ring lds 72 vs 144 at 200 rows (" + ne.tag + ", K " + std::to_string(sh.K) + ")");
          }
        }
    }
  }
  {
    Problem& P = Ps.get(513, 384, 1536);
    NamedEpi ne;
    make_epi(P, gcr::K_RESID_LN, V_OFFSET, ne);
    run_ring(F, P, ne, RingPlan{128, 128, 144, 8, true}, 1280);
  }
  free_to(1);
}

// launch_dec_oneshot (plan value -2): rows in groups of 32, K ranges of <= 1280
static void fam_oneshot(Fam& F) {
  Problems Ps;
  for (int M : {31, 32, 33, 150})
    for (int N : {384, 420})
      for (int K : {64, 384, 1280, 1536, 5120}) {
        Problem& P = Ps.get(M, N, K);
        const int s = (K / 32 + 39) / 40;
        for (const NamedEpi& ne : epis_for(P, DEC_KINDS))
          for (int nc : {2, 4}) {
            const bool ln = ne.e.kind == gcr::K_RESID_LN;
            run_case(F, P, ne, "dec_oneshot nc " + std::to_string(nc), N % 128 == 0, (s > 1 || ln) ? s : 0,
                     [nc](const GemmA& a, const bf16* w, long long ldw, int M2, int N2, int K2, const GemmEpi& e, float* ws, size_t wsb) {
                       return launch_dec_oneshot(a, w, ldw, M2, N2, K2, e, ws, wsb, nc, 0);
                     });
          }
      }
  {
    Problem& P = Ps.get(150, 384, 1536);
    NamedEpi ne;
    make_epi(P, gcr::K_RESID_LN, V_OFFSET, ne);
    run_case(F, P, ne, "dec_oneshot nc 2", true, 2,
             [](const GemmA& a, const bf16* w, long long ldw, int M2, int N2, int K2, const GemmEpi& e, float* ws, size_t wsb) {
               return launch_dec_oneshot(a, w, ldw, M2, N2, K2, e, ws, wsb, 2, 0);
             });
  }
  free_to(1);
}

// launch_dec_gemv in its plain modes (the fused-LayerNorm modes are tools/gemv_check's): M <= 32, N % 16 == 0, K % 128 == 0
static void fam_gemv(Fam& F) {
  Problems Ps;
  const Launch fn = [](const GemmA& a, const bf16* w, long long ldw, int M, int N, int K, const GemmEpi& e, float* ws, size_t wsb) {
    return launch_dec_gemv(a, w, ldw, M, N, K, e, ws, wsb, 0);
  };
  for (int M : {1, 5, 16, 17, 32})
    for (int N : {384, 400, 420})
      for (int K : {128, 384, 1280, 1536, 5120}) {
        Problem& P = Ps.get(M, N, K);
        const int s = gemv_splits(M, N, K, nullptr);
        const std::string route = "dec_gemv splits " + std::to_string(s);
        RunOut plain;
        for (const NamedEpi& ne : epis_for(P, {{gcr::K_BF16, V_PLAIN}, {gcr::K_BF16, V_GELU}, {gcr::K_RESID_F32, V_PLAIN}, {gcr::K_F32, V_PLAIN},
                                               {gcr::K_DEC_QKV, V_PLAIN}, {gcr::K_RESID_LN, V_PLAIN}})) {
          const bool ln = ne.e.kind == gcr::K_RESID_LN;
          const RunOut r = run_case(F, P, ne, route, N % 128 == 0, (s > 1 || ln) ? std::max(1, s) : 0, fn);
          if (ne.tag == "bf16") plain = r;
        }
        if (s > 1) {
          NamedEpi ne;
          make_epi(P, gcr::K_BF16, V_PLAIN, ne);
          const RunOut d = run_case(F, P, ne, route, N % 128 == 0, s, fn, true);
          expect_same(F, plain, d, "host sum of the deferred small-M slabs in split order vs the combined output");
        }
      }
  {
    Problem& P = Ps.get(16, 384, 384);
    NamedEpi ne;
    make_epi(P, gcr::K_RESID_LN, V_OFFSET, ne);
    run_case(F, P, ne, "dec_gemv", true, std::max(1, gemv_splits(16, 384, 384, nullptr)), fn);
  }
  free_to(1);
}

static const std::initializer_list<std::pair<int, int>> BIG_KINDS = {
    {gcr::K_BF16, V_GELU}, {gcr::K_BF16, V_MAP}, {gcr::K_RESID_F32, V_PLAIN}, {gcr::K_GELU_POS_F32, V_PLAIN}, {gcr::K_F32, V_PLAIN},
    {gcr::K_DEC_QKV, V_PLAIN}, {gcr::K_CROSS_KV, V_PLAIN}};
struct BigShape { int M, N, K, conv_T; };
static const BigShape BIG_SHAPES[] = {{1024, 384, 64, 0}, {1024, 384, 1280, 0}, {1025, 384, 384, 0}, {1025, 420, 384, 0}, {1500, 384, 128, 0},
                                      {1500, 420, 128, 0}, {1500, 256, 768, ROWS_PER_BATCH}, {1025, 384, 1536, 0}, {1024, 256, 5120, 0}};

// gemm_8p's persistent kernel (EPI_BF16 / RESID_F32 / F32) needs >= 2 tiles per CU: a shape of 32 x 16 tiles, with the reference on the first and
// last rows of every row tile and both sides of its middle (gathered into a plain problem); persistent off and on must
// agree in every byte of the whole output
static void p8_persistent_large(Fam& F, int K) {
  const int M = 7940, N = 3848;
  int dev = 0, cus = 0;
  CK(hipGetDevice(&dev));
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int n_tiles = ((M + 255) / 256) * ((N + 255) / 256);
  if (n_tiles < 2 * cus || cus % 8 != 0) {      // run_8p's conditions (gemm_8p.hip): else the plain kernel would run twice
    ++F.fails;
    std::printf("  FAIL        the persistent form would not be taken: %d tiles on %d CUs (needs %d tiles and CUs in eights)\n", n_tiles, cus, 2 * cus);
    return;
  }
  std::vector<int> rows;
  for (int t = 0; t * 256 < M; ++t)
    for (int o : {0, 1, 127, 128, 254, 255})
      if (t * 256 + o < M) rows.push_back(t * 256 + o);
  if (rows.back() != M - 1) rows.push_back(M - 1);
  const size_t mark = g_live.size();
  std::mt19937 rng(4242);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  std::vector<uint16_t> A((size_t)M * K), W((size_t)N * K);
  for (auto& v : A) v = gcr::f2b(U(rng));
  for (auto& v : W) v = gcr::f2b(3.f / std::sqrt((float)K) * U(rng));
  const DBuf dA = galloc("A", A.size() * 2, FILL_IN, A.data()), dW = galloc("W", W.size() * 2, FILL_IN, W.data());
  // the gathered problem: the sampled rows, plain layout
  Problem G;
  G.M = (int)rows.size(); G.N = N; G.K = K; G.ad = {K, 0, 0}; G.ldw = K;
  G.A.resize((size_t)G.M * K);
  for (int i = 0; i < G.M; ++i) std::memcpy(&G.A[(size_t)i * K], &A[(size_t)rows[i] * K], (size_t)K * 2);
  gcr::make_ref(G.A.data(), G.ad, W.data(), K, G.M, N, K, G.R);
  std::vector<float> bias(N);
  for (auto& v : bias) v = 0.1f * U(rng);
  const DBuf dbias = galloc("bias", N * 4, FILL_IN, bias.data());
  for (int kind : {gcr::K_BF16, gcr::K_RESID_F32, gcr::K_F32}) {
    const char* kname = kind == gcr::K_BF16 ? "bf16" : kind == gcr::K_F32 ? "f32" : "resid";
    const int eb = gcr::out_elem_bytes(kind);
    const long long ldc = N + 8;
    std::vector<uint8_t> init((size_t)M * ldc * eb);
    gcr::fill_sentinel(init.data(), init.size());
    gcr::Epi ge;                       // the gathered epilogue (rows i <-> rows[i])
    ge.kind = kind; ge.ldc = ldc; ge.bias = bias; ge.gelu_ulps = g_gelu_ulps;
    if (kind == gcr::K_RESID_F32) {
      ge.x_old.assign((size_t)G.M * ldc, 0.f);
      for (int r = 0; r < M; ++r) {
        float* xr = (float*)init.data() + (size_t)r * ldc;
        for (int c = 0; c < N; ++c) xr[c] = 3.f * ((float)((((uint32_t)r * 3848u + c) * 2654435761u) >> 16) / 32768.f - 1.f);
      }
      for (int i = 0; i < G.M; ++i) std::memcpy(&ge.x_old[(size_t)i * ldc], (float*)init.data() + (size_t)rows[i] * ldc, (size_t)N * 4);
    }
    gcr::Expect ex;
    gcr::build_expect(G.R, ge, ex);
    std::vector<uint8_t> got[2];
    for (int on = 0; on < 2; ++on) {
      const size_t m2 = g_live.size();
      const DBuf dout = galloc("out", init.size(), FILL_OUT, init.data());
      GemmEpi e;
      std::memset(&e, 0, sizeof(e));
      e.kind = kind; e.ldc = ldc; e.bias = (const float*)dbias.p(); e.out = dout.p();
      GemmA a;
      std::memset(&a, 0, sizeof(a));
      a.ptr = (const bf16*)dA.p(); a.ld = K;
      CK(hipMemset(g_ws.p(), FILL_WS, WSB));
      gemm_8p_set_persistent(on);
      launch_gemm_8p(a, (const bf16*)dW.p(), K, M, N, K, e, 0);
      gemm_8p_set_persistent(0);
      CK(hipDeviceSynchronize());
      got[on].resize(init.size());
      CK(hipMemcpy(got[on].data(), dout.p(), init.size(), hipMemcpyDeviceToHost));
      // sampled rows against the reference; the pad columns of every row
      std::vector<uint8_t> gath((size_t)G.M * ldc * eb);
      size_t pad_bad = 0;
      for (int i = 0; i < G.M; ++i) std::memcpy(&gath[(size_t)i * ldc * eb], &got[on][(size_t)rows[i] * ldc * eb], (size_t)ldc * eb);
      for (int r = 0; r < M; ++r)
        for (size_t b = ((size_t)r * ldc + N) * eb; b < (size_t)(r + 1) * ldc * eb; ++b) pad_bad += got[on][b] != gcr::sentinel(b);
      // the gathered image's sentinel positions differ from the full buffer's: judge the values only here
      gcr::Image vals = ex.out;
      for (int i = 0; i < G.M; ++i)
        for (int c = N; c < ldc; ++c) vals.set((size_t)i * ldc + c, gcr::elem_value(gath.data(), eb, (size_t)i * ldc + c), INFINITY);
      const gcr::Report rp = gcr::compare(vals, gath.data());
      if (!rp.ok()) print_bad("out (sampled rows)", vals, gath.data(), rp);
      const size_t ws_bad = count_ne(g_ws.p(), WSB, FILL_WS), gd = guards_damage();
      const bool k = rp.ok() && pad_bad == 0 && ws_bad == 0 && gd == 0;
      ++F.cases;
      if (!k) ++F.fails;
      Row& row = Fam::row(F.routes, std::string(on ? "gemm_8p persistent on" : "gemm_8p persistent off") + ", 512 tiles, K " + std::to_string(K) +
                                        ", sampled rows  [engine]");
      ++(k ? row.ok : row.fail);
      double w = 0;
      for (size_t i = 0; i < vals.n(); ++i)
        if (std::isfinite(vals.tol[i]) && vals.tol[i] > 0) w = std::max(w, std::fabs(gcr::elem_value(gath.data(), eb, i) - vals.v[i]) / vals.tol[i]);
      F.worst = std::max(F.worst, w);
      row.worst = std::max(row.worst, w);
      double& wt = eb == 4 ? F.worst_f32 : F.worst_bf16;
      wt = std::max(wt, w);
      if (!k || g_verbose) {
        std::printf("  %-11s %-44s %-18s M=%-4d N=%-4d K=%-4d  worst %.3f of %zu (%d sampled rows)", k ? "ok" : "FAIL",
                    on ? "gemm_8p persistent on" : "gemm_8p persistent off", kname, M, N, K, w, (size_t)G.M * N, G.M);
        if (!k) std::printf("  [%zu values, %zu pad bytes, %zu scratch bytes, %zu guard bytes]", rp.bad_val, pad_bad, ws_bad, gd);
        std::printf("\n");
      }
      free_to(m2);
    }
    ++F.exact;
    const bool same = got[0] == got[1];
    if (!same) { ++F.exact_fails; ++F.fails; }
    Row& crow = Fam::row(F.claims, "gemm_8p persistent on vs off, 512 tiles, every byte");
    ++(same ? crow.ok : crow.fail);
    if (!same || g_verbose) std::printf("  %-11s bit-identical: gemm_8p persistent on vs off, %d x %d x %d %s\n", same ? "ok" : "FAIL", M, N, K, kname);
  }
  free_to(mark);
}

static void fam_p8(Fam& F) {
  Problems Ps;
  for (const BigShape& sh : BIG_SHAPES) {
    Problem& P = Ps.get(sh.M, sh.N, sh.K, sh.conv_T);
    // (these shapes have at most 12 tiles: the persistent form needs two per CU, so only the plain kernel runs here)
    for (const NamedEpi& ne : epis_for(P, BIG_KINDS))
      run_case(F, P, ne, "gemm_8p persistent off", sh.N % 128 == 0, 0,
               [](const GemmA& a, const bf16* w, long long ldw, int M, int N, int K, const GemmEpi& e, float*, size_t) {
                 if (!gemm_8p_applicable(M, N, K)) return false;
                 gemm_8p_set_persistent(0);
                 launch_gemm_8p(a, w, ldw, M, N, K, e, 0);
                 return true;
               });
  }
  free_to(1);
  // the persistent kernel: its two-K-tile minimum (every K step at a tile seam), and K depths with in-tile steps
  for (int K : {128, 384, 1280}) p8_persistent_large(F, K);
}

static void fam_big(Fam& F) {
  Problems Ps;
  for (const BigShape& sh : BIG_SHAPES) {
    Problem& P = Ps.get(sh.M, sh.N, sh.K, sh.conv_T);
    for (const NamedEpi& ne : epis_for(P, BIG_KINDS))
      run_case(F, P, ne, "gemm_big", sh.N % 128 == 0 && sh.K >= 96, 0,
               [](const GemmA& a, const bf16* w, long long ldw, int M, int N, int K, const GemmEpi& e, float*, size_t) {
                 if (!gemm_big_applicable(M, N, K)) return false;      // the launcher itself has no guard (K >= 96)
                 launch_gemm_big(a, w, ldw, M, N, K, e, 0);
                 return true;
               });
  }
  free_to(1);
}

// launch_splitk_combine alone: slabs of random f32 partial sums in the scratch (acc = their sum, "K" = the slab count)
static void fam_combine(Fam& F) {
  for (int M : {1, 150, 600})
    for (int N : {384, 420, 1001})
      for (int splitk : {1, 2, 4, 9}) {
        Problem P;
        P.M = M; P.N = N; P.K = splitk; P.ad = {0, 0, 0}; P.ldw = 0;
        std::mt19937 rng(99u * M + N + splitk);
        std::uniform_real_distribution<float> U(-1.f, 1.f);
        std::vector<float> part((size_t)splitk * M * N);
        for (auto& v : part) v = U(rng);
        P.R.M = M; P.R.N = N; P.R.K = splitk;
        P.R.acc.assign((size_t)M * N, 0.0);
        P.R.S.assign((size_t)M * N, 0.0);
        for (int s = 0; s < splitk; ++s)
          for (size_t i = 0; i < (size_t)M * N; ++i) { P.R.acc[i] += part[s * (size_t)M * N + i]; P.R.S[i] += std::fabs(part[s * (size_t)M * N + i]); }
        const DBuf dpart = galloc("slabs", part.size() * 4, FILL_IN, part.data());
        const Launch fn = [&](const GemmA&, const bf16*, long long, int M2, int N2, int, const GemmEpi& e, float*, size_t) {
          launch_splitk_combine((const float*)dpart.p(), splitk, M2, N2, e, 0);
          return true;
        };
        for (const NamedEpi& ne : epis_for(P, {{gcr::K_BF16, V_PLAIN}, {gcr::K_BF16, V_MAP}, {gcr::K_RESID_F32, V_PLAIN}, {gcr::K_F32, V_PLAIN},
                                               {gcr::K_F32, V_MAP}, {gcr::K_DEC_QKV, V_PLAIN}, {gcr::K_RESID_LN, V_PLAIN}, {gcr::K_RESID_LN, V_OFFSET}})) {
          const RunOut r = run_case(F, P, ne, "splitk_combine of " + std::to_string(splitk), true, 0, fn);
          if (ne.tag == "f32 nobias" && r.supported) {   // summed in split order: the host's f32 sum in that order, bit for bit
            RunOut h = r;
            for (int rr = 0; rr < M; ++rr)
              for (int c = 0; c < N; ++c) {
                float v = 0.f;
                for (int s = 0; s < splitk; ++s) v += part[((size_t)s * M + rr) * N + c];
                std::memcpy(&h.out[((size_t)rr * ne.e.ldc + c) * 4], &v, 4);
              }
            expect_same(F, h, r, "combine vs the host's f32 sum in split order (M " + std::to_string(M) + " N " + std::to_string(N) + ")");
          }
        }
        free_to(1);
      }
}

// the device gelu_erf against f64 on a dense grid over [-8, 8], in units of 2^-24 max(1, |x|)
static double measure_gelu() {
  const int n = 1 << 20;
  std::vector<float> x(n), y(n);
  for (int i = 0; i < n; ++i) x[i] = (float)(-8.0 + 16.0 * i / (n - 1));
  const size_t mark = g_live.size();
  const DBuf dx = galloc("gelu x", n * 4, FILL_IN, x.data()), dy = galloc("gelu y", n * 4, FILL_OUT);
  hipLaunchKernelGGL(gelu_probe_kernel, dim3(n / 256), dim3(256), 0, 0, (const float*)dx.p(), (float*)dy.p(), n);
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(y.data(), dy.p(), n * 4, hipMemcpyDeviceToHost));
  double worst = 0, at = 0;
  for (int i = 0; i < n; ++i) {
    const double r = std::fabs((double)y[i] - gcr::gelu64((double)x[i])) / (gcr::U24 * std::max(1.0, std::fabs((double)x[i])));
    if (!(r <= worst)) { worst = r; at = x[i]; }
  }
  free_to(mark);
  std::printf("device gelu_erf vs f64 on %d points of [-8, 8]: max error %.2f x 2^-24 max(1, |x|) at x = %.4f (assumed bound %.0f)\n", n, worst,
              at, gcr::GELU_ULPS_START);
  return worst;
}

int main(int argc, char** argv) {
  struct Entry { const char* name; void (*fn)(Fam&); };
  const Entry fams[] = {{"skinny", fam_skinny}, {"tiled", fam_tiled}, {"ring", fam_ring}, {"ring_big", fam_ring_big}, {"oneshot", fam_oneshot},
                        {"gemv", fam_gemv}, {"p8", fam_p8}, {"big", fam_big}, {"combine", fam_combine}};
  const std::string want = argc > 1 ? argv[1] : "";
  g_verbose = argc > 2 && std::string(argv[2]) == "-v";
  bool known = want == "all";
  for (const Entry& e : fams) known |= want == e.name;
  if (!known) {
    std::fprintf(stderr, "usage: gemm_check skinny|tiled|ring|ring_big|oneshot|gemv|p8|big|combine|all [-v]\n");
    return 2;
  }
  std::setvbuf(stdout, nullptr, _IOLBF, 0);
  CK(hipMalloc(&g_cnt, 8));
  g_ws = galloc("split-K scratch", WSB, FILL_WS);       // g_live[0]: lives for the whole run
  const double gm = measure_gelu();
  if (!(gm <= gcr::GELU_ULPS_START)) {
    g_gelu_ulps = std::ceil(gm);
    std::printf("FAIL: the measured gelu error exceeds the assumed bound of %.0f; this run fails.  EPI_GELU_POS_F32 is judged with "
                "g = %.0f x 2^-24 max(1, |x|) below so that the rest can be read\n", gcr::GELU_ULPS_START, g_gelu_ulps);
  }
  int bad = gm <= gcr::GELU_ULPS_START ? 0 : 1;
  for (const Entry& e : fams) {
    if (want != "all" && want != e.name) continue;
    Fam F;
    F.name = e.name;
    std::printf("family %s\n", e.name);
    const auto t0 = std::chrono::steady_clock::now();
    e.fn(F);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // the family's table: per route (marked [engine] where engine.cpp produces the plan at these shapes) the cases that
    // passed / failed / were refused and the worst error / tolerance; then the bit-identity claims
    for (const Row& r : F.routes) {
      std::printf("  %-74s %4zu ok %3zu FAIL %3zu unsupported  worst %.3f", r.name.c_str(), r.ok, r.fail, r.unsupported, r.worst);
      if (r.unsupported) std::printf("  (%s)", r.why.c_str());
      std::printf("\n");
    }
    for (const Row& r : F.claims)
      std::printf("  bit-identical: %-59s %4zu ok %3zu FAIL %3zu skipped (a run refused)\n", r.name.c_str(), r.ok, r.fail, r.unsupported);
    const bool ok = F.fails == 0 && F.cases > 0;
    bad += !ok;
    std::printf("family %s: %s  (%zu cases, %zu failed, %zu unsupported of which %zu on engine-reachable plans, %zu bit-identity checks of "
                "which %zu failed, worst error / tolerance %.3f: f32 outputs %.3f, bf16 outputs %.3f, LayerNorm outputs %.3f; %.1f s)\n", e.name, ok ? "ok" : "FAIL", F.cases, F.fails, F.unsupported, F.refused,
                F.exact, F.exact_fails, F.worst, F.worst_f32, F.worst_bf16, F.worst_ln, secs);
  }
  free_to(0);
  CK(hipFree(g_cnt));
  std::printf("%s\n", bad ? "FAILURES" : "all ok");
  return bad ? 1 : 0;
}
