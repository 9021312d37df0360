// CPU self-test of tools/gemm_check_ref.h (the reference and comparator of tools/gemm_check; no GPU, no HIP):
// a "device" output is made from the reference itself, then one defect at a time is planted and the comparator
// must flag that defect and nothing else.  It also recomputes the products in f32 with a shuffled summation
// order and requires them to pass: the tolerances are not already violated by a correct f32 kernel.
//   usage: gemm_check_selftest
#include <cstdio>
#include <numeric>
#include <random>
#include <set>
#include "gemm_check_ref.h"

using namespace gcr;

static int g_fail = 0;
#define REQUIRE(cond, ...)                    \
  do {                                        \
    if (!(cond)) {                            \
      ++g_fail;                               \
      std::printf("  FAIL %s: ", #cond);      \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
    }                                         \
  } while (0)

// the bytes a faultless device would leave: the sentinel, the reference value (rounded to the output type) where written
static std::vector<uint8_t> device_like(const Image& im) {
  std::vector<uint8_t> b(im.bytes());
  fill_sentinel(b.data(), b.size());
  for (size_t i = 0; i < im.n(); ++i)
    if (im.w[i]) {
      if (im.elem == 2) { const uint16_t h = f2b((float)im.v[i]); std::memcpy(&b[i * 2], &h, 2); }
      else { const float f = (float)im.v[i]; std::memcpy(&b[i * 4], &f, 4); }
    }
  return b;
}

struct Problem {
  int M, N, K;
  ADesc ad;
  std::vector<uint16_t> A, W;
  Ref R;
};

int main() {
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  Problem P{40, 96, 384, {384, 0, 0}};
  P.A.resize(a_elems(P.ad, P.M, P.K));
  P.W.resize((size_t)P.N * P.K);
  for (auto& v : P.A) v = f2b(U(rng));
  for (auto& v : P.W) v = f2b(3.f / std::sqrt((float)P.K) * U(rng));
  make_ref(P.A.data(), P.ad, P.W.data(), P.K, P.M, P.N, P.K, P.R);
  const int M = P.M, N = P.N, K = P.K;

  auto base = [&](int kind) {
    Epi e;
    e.kind = kind;
    e.ldc = N + 8;                       // 8 pad columns
    e.bias.resize(N);
    for (auto& v : e.bias) v = 0.1f * U(rng);
    return e;
  };
  Epi ebf = base(K_BF16);
  ebf.act = 1; ebf.rpb = 16; ebf.roff = 1; ebf.bstride = 17 * ebf.ldc;
  Epi ef32 = base(K_F32);
  Epi ers = base(K_RESID_F32);
  ers.x_old.resize((size_t)M * ers.ldc);
  for (auto& v : ers.x_old) v = 3.f * U(rng);
  Epi egp = base(K_GELU_POS_F32);
  egp.rpb = 16;
  egp.pos.resize((size_t)egp.rpb * egp.ldc);
  for (auto& v : egp.pos) v = U(rng);
  Epi eq = base(K_DEC_QKV);
  eq.d = 32; eq.head_dim = 16; eq.n_head = 2; eq.n_ctx = 7; eq.n_hyp = 8;
  for (int r = 0; r < M; ++r) { const int s = (r * 5 + 3) % 56; eq.row_hyp.push_back(s / 7); eq.row_pos.push_back(s % 7); }
  Epi ec = base(K_CROSS_KV);
  ec.d = 48; ec.head_dim = 16; ec.n_head = 3; ec.rpb = 16; ec.n_slots = 4; ec.slot0 = 1;

  std::printf("clean copies of the reference pass\n");
  for (const Epi* e : {&ebf, &ef32, &ers, &egp, &eq, &ec}) {
    Expect x;
    build_expect(P.R, *e, x);
    for (const Image* im : {&x.out, &x.kc, &x.vc}) {
      if (!im->n()) continue;
      const Report rp = compare(*im, device_like(*im).data());
      REQUIRE(rp.ok() && rp.bad.empty(), "kind %d: %zu values, %zu sentinels flagged", e->kind, rp.bad_val, rp.bad_sentinel);
      REQUIRE(rp.checked > 0 && rp.worst <= 1.0, "kind %d worst %g", e->kind, rp.worst);
    }
    size_t written = 0;
    for (uint8_t w : x.out.w) written += w;
    for (uint8_t w : x.kc.w) written += w;
    for (uint8_t w : x.vc.w) written += w;
    REQUIRE(written == (size_t)M * N, "kind %d writes %zu elements, not M N", e->kind, written);
  }

  std::printf("an f32 recomputation in a shuffled summation order passes\n");
  {
    std::vector<int> perm(K);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<float> accf((size_t)M * N);
    for (int r = 0; r < M; ++r)
      for (int c = 0; c < N; ++c) {
        float s = 0.f;
        for (int k : perm) s += b2f(P.A[a_off(P.ad, r) + k]) * b2f(P.W[(size_t)c * K + k]);
        accf[(size_t)r * N + c] = s;
      }
    auto gelf = [](float x) { return 0.5f * x * (1.0f + std::erf(x * 0.70710678118654752f)); };
    for (const Epi* e : {&ebf, &ef32, &ers, &egp}) {
      Expect x;
      build_expect(P.R, *e, x);
      std::vector<uint8_t> b = device_like(x.out);
      for (int r = 0; r < M; ++r)
        for (int c = 0; c < N; ++c) {
          const float v = accf[(size_t)r * N + c] + e->bias[c];
          if (e->kind == K_BF16) {
            const size_t o = (size_t)(r / e->rpb) * e->bstride + (size_t)(r % e->rpb + e->roff) * e->ldc + c;
            const uint16_t h = f2b(gelf(v));
            std::memcpy(&b[o * 2], &h, 2);
          } else {
            const size_t o = (size_t)r * e->ldc + c;
            float f = v;
            if (e->kind == K_RESID_F32) f = e->x_old[o] + v;
            if (e->kind == K_GELU_POS_F32) f = gelf(v) + e->pos[(size_t)(r % e->rpb) * e->ldc + c];
            std::memcpy(&b[o * 4], &f, 4);
          }
        }
      const Report rp = compare(x.out, b.data());
      std::printf("  kind %d: worst error / tolerance %.3f\n", e->kind, rp.worst);
      REQUIRE(rp.ok(), "kind %d: %zu of %zu out of tolerance, worst %g", e->kind, rp.bad_val, rp.checked, rp.worst);
    }
  }

  std::printf("defect: one bf16 element off by two ulps\n");
  {
    Epi e = base(K_BF16);
    Expect x;
    build_expect(P.R, e, x);
    for (int sign : {+2, -2}) {
      // a sample of a hundred written elements, spread over the magnitudes
      std::vector<size_t> idx;
      for (size_t i = 0; i < x.out.n(); ++i) if (x.out.w[i]) idx.push_back(i);
      std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return std::fabs(x.out.v[a]) > std::fabs(x.out.v[b]); });
      size_t caught = 0, tried = 0;
      for (size_t j = 0; j < idx.size(); j += std::max<size_t>(1, idx.size() / 100)) {
        std::vector<uint8_t> b = device_like(x.out);
        uint16_t h;
        std::memcpy(&h, &b[idx[j] * 2], 2);
        h = (uint16_t)(h + sign);
        std::memcpy(&b[idx[j] * 2], &h, 2);
        const Report rp = compare(x.out, b.data());
        ++tried;
        caught += rp.bad_val == 1 && rp.bad_sentinel == 0 && rp.bad.size() == 1 && rp.bad[0] == idx[j];
        REQUIRE(rp.bad_val <= 1 && rp.bad_sentinel == 0, "another element was flagged");
      }
      // an element whose own tolerance E exceeds its bf16 ulp (a value near zero after cancellation) cannot show two
      // ulps (here |v| < 0.044, a few percent of the elements), so the largest element and nine in ten are required
      std::printf("  %+d ulps: caught at %zu of %zu sampled elements\n", sign, caught, tried);
      std::vector<uint8_t> b = device_like(x.out);
      uint16_t h;
      std::memcpy(&h, &b[idx[0] * 2], 2);
      h = (uint16_t)(h + sign);
      std::memcpy(&b[idx[0] * 2], &h, 2);
      const Report rp = compare(x.out, b.data());
      REQUIRE(rp.bad_val == 1 && rp.bad.size() == 1 && rp.bad[0] == idx[0], "largest element not flagged");
      REQUIRE(caught * 10 >= tried * 9, "two ulps caught at only %zu of %zu elements", caught, tried);
    }
  }

  std::printf("defect: one f32 element off by 4 E\n");
  for (const Epi* e : {&ef32, &ers}) {
    Expect x;
    build_expect(P.R, *e, x);
    size_t caught = 0, tried = 0;
    for (int r = 0; r < M; r += 3)
      for (int c = 0; c < N; c += 7) {
        const size_t i = (size_t)r * N + c, o = (size_t)r * e->ldc + c;
        const double xo = e->kind == K_RESID_F32 ? std::fabs(e->x_old[o]) : 0.0;
        const double E = (K + 8) * U24 * (P.R.S[i] + std::fabs(e->bias[c]) + xo);
        std::vector<uint8_t> b = device_like(x.out);
        const float f = (float)(x.out.v[o] + 4 * E);
        std::memcpy(&b[o * 4], &f, 4);
        const Report rp = compare(x.out, b.data());
        ++tried;
        caught += rp.bad_val == 1 && rp.bad_sentinel == 0 && rp.bad.size() == 1 && rp.bad[0] == o;
      }
    REQUIRE(caught == tried, "kind %d: caught %zu of %zu", e->kind, caught, tried);
  }

  std::printf("defect: one dropped K-tile in one row\n");
  for (const Epi* e : {&ef32, &ebf}) {
    Expect x;
    build_expect(P.R, *e, x);
    const int r = 23;
    Ref R1;                               // row r without its last 64 k
    make_ref(P.A.data() + a_off(P.ad, r), P.ad, P.W.data(), K, 1, N, K - 64, R1);
    Ref R2 = P.R;
    for (int c = 0; c < N; ++c) R2.acc[(size_t)r * N + c] = R1.acc[c];
    Expect y;
    build_expect(R2, *e, y);
    const Report rp = compare(x.out, device_like(y.out).data());
    std::set<size_t> rowset;
    for (int c = 0; c < N; ++c)
      rowset.insert(e->kind == K_BF16 ? (size_t)(r / e->rpb) * e->bstride + (size_t)(r % e->rpb + e->roff) * e->ldc + c
                                      : (size_t)r * e->ldc + c);
    bool inside = true;
    for (size_t i : rp.bad) inside &= rowset.count(i) == 1;
    std::printf("  kind %d: %zu of %d elements of the row flagged\n", e->kind, rp.bad_val, N);
    REQUIRE(inside && rp.bad_sentinel == 0, "an element outside the row was flagged");
    REQUIRE(rp.bad_val * 10 >= (size_t)N * 9, "only %zu of %d flagged", rp.bad_val, N);
  }

  std::printf("defect: two K/V rows scattered to each other's slot\n");
  {
    Expect x;
    build_expect(P.R, eq, x);
    const int r1 = 4, r2 = 29;
    Epi sw = eq;
    std::swap(sw.row_hyp[r1], sw.row_hyp[r2]);
    std::swap(sw.row_pos[r1], sw.row_pos[r2]);
    Expect y;
    build_expect(P.R, sw, y);
    const Report rq = compare(x.out, device_like(y.out).data());
    REQUIRE(rq.ok(), "the q part does not depend on the row maps");
    for (int kv = 0; kv < 2; ++kv) {
      const Report rp = compare(kv ? x.vc : x.kc, device_like(kv ? y.vc : y.kc).data());
      std::set<size_t> slots;
      for (int r : {r1, r2})
        for (int h = 0; h < eq.n_head; ++h)
          for (int e2 = 0; e2 < eq.head_dim; ++e2)
            slots.insert((((size_t)eq.row_hyp[r] * eq.n_head + h) * eq.n_ctx + eq.row_pos[r]) * eq.head_dim + e2);
      bool inside = true;
      for (size_t i : rp.bad) inside &= slots.count(i) == 1;
      std::printf("  %s cache: %zu of %zu elements of the two rows flagged\n", kv ? "v" : "k", rp.bad_val, slots.size());
      REQUIRE(inside && rp.bad_sentinel == 0, "an element outside the two rows was flagged");
      REQUIRE(rp.bad_val * 10 >= slots.size() * 9, "only %zu of %zu flagged", rp.bad_val, slots.size());
    }
  }

  std::printf("defect: one sentinel byte changed in an ldc pad\n");
  for (const Epi* e : {&ebf, &ef32, &ers}) {
    Expect x;
    build_expect(P.R, *e, x);
    std::vector<uint8_t> b = device_like(x.out);
    const size_t el = (e->kind == K_BF16 ? (size_t)e->roff * e->ldc : 0) + 5 * e->ldc + N + 2;   // a pad column
    REQUIRE(!x.out.w[el], "element %zu is not a pad", el);
    b[el * x.out.elem + 1] ^= 0x10;
    const Report rp = compare(x.out, b.data());
    REQUIRE(rp.bad_sentinel == 1 && rp.bad_val == 0 && rp.bad.size() == 1 && rp.bad[0] == el, "kind %d: %zu sentinels, %zu values",
            e->kind, rp.bad_sentinel, rp.bad_val);
  }
  {                                       // row 0 of a roff = 1 block is never written either
    Expect x;
    build_expect(P.R, ebf, x);
    std::vector<uint8_t> b = device_like(x.out);
    const size_t el = (size_t)ebf.bstride + 3;
    REQUIRE(!x.out.w[el], "row 0 of block 1 is written");
    b[el * 2] ^= 1;
    const Report rp = compare(x.out, b.data());
    REQUIRE(rp.bad_sentinel == 1 && rp.bad.size() == 1 && rp.bad[0] == el, "row 0 of a block not watched");
  }

  std::printf("defect: one guard byte changed\n");
  {
    std::vector<uint8_t> g(1 << 16, 0x5a);
    size_t first = 0;
    REQUIRE(guard_damage(g.data(), g.size(), 0x5a) == 0, "a clean guard reported");
    g[4711] = 0x5b;
    REQUIRE(guard_damage(g.data(), g.size(), 0x5a, &first) == 1 && first == 4711, "guard byte not found");
  }

  std::printf("defect: ln_out from a one-pass variance, residual offset 1000\n");
  for (float offset : {0.f, 1000.f}) {
    const int LM = 8, LN = 384;
    Epi e;
    e.kind = K_RESID_LN;
    e.ln_ld = LN + 8;
    e.ln_g.resize(LN);
    e.ln_b.resize(LN);
    for (auto& v : e.ln_g) v = 1.f + 0.2f * U(rng);
    for (auto& v : e.ln_b) v = 0.1f * U(rng);
    std::vector<float> xs((size_t)LM * LN);
    for (auto& v : xs) v = offset + 3.f * U(rng);
    Image im;
    build_ln_expect(xs.data(), LN, LM, LN, e, im);
    for (int one_pass = 0; one_pass < 2; ++one_pass) {
      std::vector<uint8_t> b = device_like(im);
      for (int r = 0; r < LM; ++r) {
        const float* xr = &xs[(size_t)r * LN];
        float s = 0.f, q = 0.f;
        for (int c = 0; c < LN; ++c) s += xr[c];
        const float mean = s / LN;
        if (one_pass) {
          for (int c = 0; c < LN; ++c) q += xr[c] * xr[c];
          q = q / LN - mean * mean;
        } else {
          for (int c = 0; c < LN; ++c) q += (xr[c] - mean) * (xr[c] - mean);
          q /= LN;
        }
        const float rstd = 1.0f / std::sqrt(q + 1e-5f);
        for (int c = 0; c < LN; ++c) {
          const uint16_t h = f2b((xr[c] - mean) * rstd * e.ln_g[c] + e.ln_b[c]);
          std::memcpy(&b[((size_t)r * e.ln_ld + c) * 2], &h, 2);
        }
      }
      const Report rp = compare(im, b.data());
      std::printf("  offset %4.0f %s: %zu of %zu flagged, worst %.3g\n", offset, one_pass ? "one-pass" : "two-pass", rp.bad_val,
                  rp.checked, rp.worst);
      if (!one_pass) REQUIRE(rp.ok(), "a correct two-pass f32 LayerNorm fails (worst %g)", rp.worst);
      if (one_pass && offset > 0) REQUIRE(rp.bad_val > 0 && rp.bad_sentinel == 0, "the one-pass variance passed");
    }
  }

  std::printf("%s\n", g_fail ? "SELFTEST FAILURES" : "selftest ok");
  return g_fail ? 1 : 0;
}
