// CPU self-test of tools/attn_check_ref.h (host compiler, no HIP): proves without a GPU that the check accepts a
// correct kernel and rejects a subtly wrong one.
//   (a) plain-C++ f32 emulations of the two algorithms the decoder attention kernels use must pass on every input
//       generator with an error / tolerance ratio <= 0.5 (the bounds are doubled rounding-step counts).  The ratio
//       is taken on the f32 result; after the final bf16 store it must stay <= 1: the store's own error reaches
//       2^-8 |x| (bf16 keeps 8 significant bits), which is the whole of the 2 U9 |ref| term, so that term has no
//       margin to halve.
//         one-pass online softmax in 128 / 64-key chunks, 8 lane groups merged pairwise, segments (waves of the
//         KSPLIT form, key splits of the group kernel) merged with weights 2^(m_s - M)
//         deferred-rescale tiles of 32 and of 64 keys, P rounded to bf16, f32 l, bf16 u / l partials merged with
//         l_s 2^(m_s - M) / L; the rows of a tile share one wave-wide `any` vote
//   (b) seeded faults must be rejected on the forcing inputs; on the plain randn-scale input the rescale faults are
//       accepted (the branch fires only on the first tile, where l = o = 0), which is why a suite on bounded random
//       data cannot see them.  The other faults are reported on plain too (most are visible to these bounds even
//       there; they hide only under the wider whole-model tolerances).
//   (c) the blocked-slot, xswap23 and partial-record layouts round-trip against direct index formulas.
#define ATTN_H_CONSTANTS_ONLY
#include "../vlog_amd/csrc/attn.h"
#include "attn_check_ref.h"

#include <cstdio>
#include <string>

using namespace acr;

static int g_fail = 0;
#define EXPECT(c, ...)                                   \
  do {                                                   \
    if (!(c)) { ++g_fail; std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); } \
  } while (0)

static const float SL2 = 0.125f * 1.4426950408889634f;

// the 8-lane dot product of the VALU kernels: 8 FMA chains of 8 elements, summed by xor-shuffles 1, 2, 4
static float dot8x8(const float* qs, const float* k) {
  float s[8];
  for (int sub = 0; sub < 8; ++sub) {
    float d = 0.f;
    for (int i = 0; i < 8; ++i) d = std::fmaf(qs[sub * 8 + i], k[sub * 8 + i], d);
    s[sub] = d;
  }
  return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

struct OnePassFault { bool no_mask = false, merge_no_m = false; };
// segs: the key row indices each segment (wave / split) walks; out = the f32 result before its bf16 rounding
static void emu_onepass(const float* q, const float* K, const float* V, const std::vector<std::vector<long long>>& segs,
                        OnePassFault f, float* out) {
  float qs[HD];
  for (int i = 0; i < HD; ++i) qs[i] = q[i] * SL2;
  const int S = (int)segs.size();
  std::vector<float> sm(S), sl(S), so((size_t)S * HD);
  for (int w = 0; w < S; ++w) {
    const auto& kl = segs[w];
    const int n = (int)kl.size();
    float m[8], l[8], o[8][HD];
    for (int g = 0; g < 8; ++g) { m[g] = -INFINITY; l[g] = 0.f; for (int e = 0; e < HD; ++e) o[g][e] = 0.f; }
    for (int kb = 0; kb < n;) {
      const int U = n - kb > 64 ? 16 : 8;
      for (int g = 0; g < 8; ++g) {
        float sc[16];
        const float* vr[16];
        float mx = m[g];
        for (int u = 0; u < U; ++u) {
          const int p = kb + u * 8 + g;
          const bool ok = p < n;
          const long long row = kl[ok ? p : 0];           // the kernels clamp a masked key's address to key 0
          sc[u] = (ok || f.no_mask) ? dot8x8(qs, K + row * HD) : -INFINITY;
          vr[u] = V + row * HD;
          mx = std::fmax(mx, sc[u]);
        }
        const float ms = mx == -INFINITY ? 0.f : mx;
        const float corr = std::exp2(m[g] - ms);
        float pu[16], ps = 0.f;
        for (int u = 0; u < U; ++u) { pu[u] = std::exp2(sc[u] - ms); ps += pu[u]; }
        l[g] = l[g] * corr + ps;
        for (int e = 0; e < HD; ++e) {
          float x = o[g][e] * corr;
          for (int u = 0; u < U; ++u) x = std::fmaf(pu[u], vr[u][e], x);
          o[g][e] = x;
        }
        m[g] = mx;
      }
      kb += U * 8;
    }
    for (int off = 1; off < 8; off <<= 1)
      for (int g = 0; g < 8; g += 2 * off) {
        const int h = g + off;
        const float M = std::fmax(m[g], m[h]), Ms = M == -INFINITY ? 0.f : M;
        const float ca = std::exp2(m[g] - Ms), cb = std::exp2(m[h] - Ms);
        l[g] = l[g] * ca + l[h] * cb;
        for (int e = 0; e < HD; ++e) o[g][e] = o[g][e] * ca + o[h][e] * cb;
        m[g] = M;
      }
    sm[w] = m[0]; sl[w] = l[0];
    for (int e = 0; e < HD; ++e) so[(size_t)w * HD + e] = o[0][e];
  }
  float M = -INFINITY;
  for (int w = 0; w < S; ++w) M = std::fmax(M, sm[w]);
  float L = 0.f, O[HD] = {0.f};
  for (int w = 0; w < S; ++w) {
    const float c = f.merge_no_m ? 1.f : std::exp2(sm[w] - M);
    L += sl[w] * c;
    for (int e = 0; e < HD; ++e) O[e] += so[(size_t)w * HD + e] * c;
  }
  for (int e = 0; e < HD; ++e) out[e] = O[e] / L;      // (the kernel then rounds to bf16: round_out)
}
static void round_out(float* o) {
  for (int e = 0; e < HD; ++e) o[e] = rb(o[e]);
}

struct DeferredFault { bool no_l = false, no_m = false, alpha_other = false, no_mask = false, merge_no_m = false; };
// R rows share every tile's `any` vote.  out [R][HD] f32 (the merged u of xcomb_vo before its hi + lo split);
// m_out / l_out [R][splits] are the partials' (m, l).
static void emu_deferred(const float* Q, int R, const float* K, const float* V, int T, int KT, int splits, DeferredFault f,
                         float thr, float* out, std::vector<float>& m_out, std::vector<float>& l_out) {
  const int ntt = (T + KT - 1) / KT;
  std::vector<float> pu((size_t)R * splits * HD);
  m_out.assign((size_t)R * splits, 0.f);
  l_out.assign((size_t)R * splits, 0.f);
  for (int sp = 0; sp < splits; ++sp) {
    const int tb = sp * ntt / splits, te = (sp + 1) * ntt / splits;
    std::vector<float> m_run(R, -INFINITY), l_run(R, 0.f), o((size_t)R * HD, 0.f), sc((size_t)R * KT), mx(R);
    for (int t = tb; t < te; ++t) {
      bool any = false;
      for (int r = 0; r < R; ++r) {
        mx[r] = -INFINITY;
        for (int j = 0; j < KT; ++j) {
          const int key = t * KT + j;
          float s = -INFINITY;
          if (key < T || f.no_mask) {
            const float* k = K + (size_t)std::min(key, T - 1) * HD;
            float d = 0.f;
            for (int i = 0; i < HD; ++i) d = std::fmaf(k[i], Q[r * HD + i], d);   // the MFMA's f32 accumulation
            s = d * SL2;
          }
          sc[(size_t)r * KT + j] = s;
          mx[r] = std::fmax(mx[r], s);
        }
        any |= mx[r] > m_run[r] + thr;
      }
      if (any) {
        std::vector<float> alpha(R), mn(R);
        for (int r = 0; r < R; ++r) { mn[r] = std::fmax(m_run[r], mx[r]); alpha[r] = std::exp2(m_run[r] - mn[r]); }
        for (int r = 0; r < R; ++r) {
          const float a = alpha[f.alpha_other ? (r + 1) % R : r];
          if (!f.no_l) l_run[r] *= a;
          for (int e = 0; e < HD; ++e) o[(size_t)r * HD + e] *= a;
          if (!(f.no_m && m_run[r] != -INFINITY)) m_run[r] = mn[r];
        }
      }
      for (int r = 0; r < R; ++r)
        for (int j = 0; j < KT; ++j) {
          const float p = std::exp2(sc[(size_t)r * KT + j] - m_run[r]);
          l_run[r] += p;
          const float pb = rb(p);
          if (pb == 0.f) continue;
          const float* v = V + (size_t)std::min(t * KT + j, T - 1) * HD;
          for (int e = 0; e < HD; ++e) o[(size_t)r * HD + e] = std::fmaf(pb, v[e], o[(size_t)r * HD + e]);
        }
    }
    for (int r = 0; r < R; ++r) {
      m_out[(size_t)r * splits + sp] = m_run[r];
      l_out[(size_t)r * splits + sp] = l_run[r];
      const float inv = 1.0f / l_run[r];
      for (int e = 0; e < HD; ++e) pu[((size_t)r * splits + sp) * HD + e] = rb(o[(size_t)r * HD + e] * inv);
    }
  }
  for (int r = 0; r < R; ++r) {
    float M = -INFINITY, L = 0.f, w[16];
    for (int s = 0; s < splits; ++s) M = std::fmax(M, m_out[(size_t)r * splits + s]);
    for (int s = 0; s < splits; ++s) {
      w[s] = l_out[(size_t)r * splits + s] * (f.merge_no_m ? 1.f : std::exp2(m_out[(size_t)r * splits + s] - M));
      L += w[s];
    }
    const float inv = 1.0f / L;
    for (int e = 0; e < HD; ++e) {
      float u = 0.f;
      for (int s = 0; s < splits; ++s) u = std::fmaf(w[s] * inv, pu[((size_t)r * splits + s) * HD + e], u);
      out[r * HD + e] = u;
    }
  }
}

// ---- shared inputs: one K / V panel of T = 1500 keys (cross form) and a 5-hypothesis self cache of 448 positions
struct Panel {
  int T = 0, rows = 0;
  std::vector<float> Kf, Vf;
  std::vector<double> Kd, Vd;
};
static void make_panel(Panel& p, int rows, int T, bool by_pos_T, double thr, const std::vector<int>& bounds, bool plain_v,
                       uint64_t seed) {
  p.T = T; p.rows = rows;
  p.Kf.resize((size_t)rows * HD); p.Vf.resize((size_t)rows * HD); p.Kd.resize(p.Kf.size()); p.Vd.resize(p.Vf.size());
  Rng g(seed);
  std::vector<uint16_t> k(HD), v(HD);
  for (int r = 0; r < rows; ++r) {
    gen_key_row(g, by_pos_T ? r % T : r, T, thr, bounds, HD, k.data());
    gen_val_row(g, HD, plain_v, v.data());
    for (int e = 0; e < HD; ++e) {
      p.Kd[(size_t)r * HD + e] = p.Kf[(size_t)r * HD + e] = b2f(k[e]);
      p.Vd[(size_t)r * HD + e] = p.Vf[(size_t)r * HD + e] = b2f(v[e]);
    }
  }
}
static void make_q(int gen, uint64_t seed, float* qf, double* qd) {
  Rng g(seed);
  uint16_t q[HD];
  gen_query(g, gen, HD, 8.0, q);
  for (int e = 0; e < HD; ++e) qd[e] = qf[e] = b2f(q[e]);
}

// error / tolerance of `got` [HD] against the reference over `keys`
static double ratio_vs_ref(const double* qd, const Panel& p, const std::vector<long long>& keys, const float* got, bool p_bf16,
                           bool partial_bf16) {
  Att a;
  attend(qd, HD, scale_log2(), p.Kd.data(), HD, p.Vd.data(), HD, HD, keys.data(), (int)keys.size(), HD, a);
  Worst w;
  for (int e = 0; e < HD; ++e) {
    const double tol = tol_out(a.o[e], a.A[e], a.ds, a.n, p_bf16, a.vmax[e]) + (partial_bf16 ? 2 * U9 * a.A[e] : 0.0);
    w.see(std::fabs((double)got[e] - a.o[e]), tol, e);
  }
  return w.ratio;
}

static std::vector<long long> iota(int n) {
  std::vector<long long> v(n);
  for (int i = 0; i < n; ++i) v[i] = i;
  return v;
}
static std::vector<std::vector<long long>> cut(const std::vector<long long>& keys, int S, bool ksplit) {
  const int n = (int)keys.size();
  std::vector<std::vector<long long>> segs(S);
  const int chunk = (n + S - 1) / S;
  for (int w = 0; w < S; ++w) {
    const int b = ksplit ? w * n / S : std::min(n, w * chunk), e = ksplit ? (w + 1) * n / S : std::min(n, b + chunk);
    segs[w].assign(keys.begin() + b, keys.begin() + e);
  }
  return segs;
}

int main() {
  const float thr = XATTN_RESCALE_THR;
  static_assert(XATTN_RESCALE_THR == CROSS_TF_RESCALE_THR, "one threshold for both deferred-rescale kernels");
  const int T = 1500;
  // split bounds for EDGES: the 12 x 125-key splits of the group kernel and the 64-key-tile splits agree on multiples of
  // 500 only, so the spikes sit on the 125-key grid (first / last key of each of 12 splits)
  std::vector<int> bounds;
  for (int s = 0; s < 12; ++s) bounds.push_back(125 * s);
  Panel forcing, plain;
  make_panel(forcing, T, T, false, thr, bounds, false, 11);
  make_panel(plain, T, T, false, thr, bounds, true, 12);
  const auto all = iota(T);

  // ---------------- (a) + (b): one-pass online softmax (cross form: 1, 4 KSPLIT-style and 12 split segments)
  double worst_a1 = 0, worst_a1b = 0;
  enum { F1_NONE, F1_NOMASK, F1_DROP_LAST, F1_DUP_FIRST, F1_MERGE, F1_N };
  const char* f1_name[] = {"", "ragged chunk keys >= n not masked", "last key of a split dropped", "first key of a split read twice",
                           "merge ignores m_s (weights l_s / L)"};
  bool f1_rej[F1_N] = {false}, f1_plain_ok[F1_N];
  double f1_plain_ratio[F1_N] = {0};
  for (int fault = 0; fault < F1_N; ++fault) {
    f1_plain_ok[fault] = true;
    for (int gen = 0; gen < N_GEN; ++gen)
      for (int S : {1, 4, 12}) {
        const Panel& p = gen == PLAIN ? plain : forcing;
        float qf[HD], out[HD];
        double qd[HD];
        make_q(gen, 100 + gen, qf, qd);
        auto segs = cut(all, S, S == 4);
        OnePassFault f;
        f.no_mask = fault == F1_NOMASK;
        f.merge_no_m = fault == F1_MERGE;
        if (fault == F1_DROP_LAST) for (auto& s : segs) s.pop_back();
        if (fault == F1_DUP_FIRST) for (auto& s : segs) s.insert(s.begin(), s[0]);
        emu_onepass(qf, p.Kf.data(), p.Vf.data(), segs, f, out);
        const double r32 = ratio_vs_ref(qd, p, all, out, false, false);
        round_out(out);
        const double r = ratio_vs_ref(qd, p, all, out, false, false);
        if (fault == F1_NONE) {
          worst_a1 = std::max(worst_a1, r32);
          worst_a1b = std::max(worst_a1b, r);
          EXPECT(r32 <= 0.5 && r <= 1.0, "one-pass emulation %s S=%d ratio %.3f (bf16 %.3f)", gen_name(gen), S, r32, r);
        } else if (gen == PLAIN) {
          f1_plain_ratio[fault] = std::max(f1_plain_ratio[fault], r);
          if (r > 1.0) f1_plain_ok[fault] = false;
        } else if (r > 1.0) f1_rej[fault] = true;
      }
  }
  std::printf("emulation: one-pass online softmax, worst error/tolerance %.3f (after the bf16 store %.3f)\n", worst_a1, worst_a1b);
  for (int fault = 1; fault < F1_N; ++fault) {
    std::printf("defect: %s: forcing %s, plain %s (ratio %.2f)\n", f1_name[fault], f1_rej[fault] ? "rejected" : "ACCEPTED",
                f1_plain_ok[fault] ? "accepted" : "rejected", f1_plain_ratio[fault]);
    EXPECT(f1_rej[fault], "defect not caught: %s", f1_name[fault]);
  }

  // ---------------- self form: lineage, row_pos + 1, through a 5-hypothesis cache of 448 positions
  {
    const int NC = 448, NH = 5;
    Panel cf, cp;
    make_panel(cf, NH * NC, NC, true, thr, {0, 112, 224, 336}, false, 21);
    make_panel(cp, NH * NC, NC, true, thr, {0, 112, 224, 336}, true, 22);
    double worst = 0, worstb = 0;
    bool rej_lin = false, rej_pos = false, plain_lin = true, plain_pos = true;
    for (int gen = 0; gen < N_GEN; ++gen)
      for (int nk : {1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 447, 448}) {
        // the levels are functions of the position and of n_ctx; LAST / FIRST runner-up sit at position 447, so those
        // generators are exercised at nk = 448 and reduce to their prefix elsewhere
        const Panel& p = gen == PLAIN ? cp : cf;
        float qf[HD], out[HD];
        double qd[HD];
        make_q(gen, 200 + gen, qf, qd);
        std::vector<long long> keys(nk), ident(nk);
        for (int q = 0; q < nk; ++q) { keys[q] = (long long)(1 + q % 4) * NC + q; ident[q] = q; }   // hypothesis 0: never its own slot
        for (int S : {1, 4}) {
          emu_onepass(qf, p.Kf.data(), p.Vf.data(), cut(keys, S, true), {}, out);
          const double r32 = ratio_vs_ref(qd, p, keys, out, false, false);
          round_out(out);
          const double r = ratio_vs_ref(qd, p, keys, out, false, false);
          worst = std::max(worst, r32);
          worstb = std::max(worstb, r);
          EXPECT(r32 <= 0.5 && r <= 1.0, "self emulation %s nk=%d S=%d ratio %.3f (bf16 %.3f)", gen_name(gen), nk, S, r32, r);
        }
        emu_onepass(qf, p.Kf.data(), p.Vf.data(), cut(ident, 1, true), {}, out);
        round_out(out);
        const double rl = ratio_vs_ref(qd, p, keys, out, false, false);
        if (gen == PLAIN) plain_lin &= rl <= 1.0; else rej_lin |= rl > 1.0;
        if (nk > 1) {
          std::vector<long long> fewer(keys.begin(), keys.end() - 1);
          emu_onepass(qf, p.Kf.data(), p.Vf.data(), cut(fewer, 1, true), {}, out);
          round_out(out);
          const double rp = ratio_vs_ref(qd, p, keys, out, false, false);
          if (gen == PLAIN) plain_pos &= rp <= 1.0; else rej_pos |= rp > 1.0;
        }
      }
    std::printf("emulation: self-attention key lists, worst error/tolerance %.3f (after the bf16 store %.3f)\n", worst, worstb);
    std::printf("defect: lineage read as identity: forcing %s, plain %s\n", rej_lin ? "rejected" : "ACCEPTED", plain_lin ? "accepted" : "rejected");
    std::printf("defect: row_pos taken without the +1: forcing %s, plain %s\n", rej_pos ? "rejected" : "ACCEPTED", plain_pos ? "accepted" : "rejected");
    EXPECT(rej_lin, "defect not caught: lineage read as identity");
    EXPECT(rej_pos, "defect not caught: row_pos without the +1");
  }

  // ---------------- (a) + (b): deferred-rescale tiles of 32 and 64 keys
  {
    enum { F2_NONE, F2_NO_L, F2_NO_M, F2_ALPHA, F2_NOMASK, F2_MERGE, F2_N };
    const char* name[] = {"", "rescale branch does not scale l_run", "rescale branch scales o but leaves m_run unchanged",
                          "rescale applied with another lane's mx (alpha not per lane)", "keys >= T of the ragged tile not masked",
                          "merge ignores m_s (weights l_s / L)"};
    const bool must_hide_on_plain[] = {false, true, true, true, false, false};
    double worst = 0, worst_inv = 0;
    for (int fault = 0; fault < F2_N; ++fault) {
      bool rej = false, plain_ok = true;
      double plain_ratio = 0;
      // tiles: rows of one generator each, then MIXED (every generator, FLAT included, in one tile)
      for (int cfg = 0; cfg <= N_GEN; ++cfg) {
        const bool mixed = cfg == N_GEN;
        const int R = mixed ? N_GEN : 3;
        const Panel& p = cfg == PLAIN ? plain : forcing;
        std::vector<float> Q((size_t)R * HD), out((size_t)R * HD), mo, lo;
        std::vector<double> Qd((size_t)R * HD);
        for (int r = 0; r < R; ++r) make_q(mixed ? mixed_gen(r) : cfg, 300 + 16 * cfg + r, &Q[(size_t)r * HD], &Qd[(size_t)r * HD]);
        for (int KT : {32, 64})
          for (int S : {1, 3, 12}) {
            DeferredFault f;
            f.no_l = fault == F2_NO_L; f.no_m = fault == F2_NO_M; f.alpha_other = fault == F2_ALPHA;
            f.no_mask = fault == F2_NOMASK; f.merge_no_m = fault == F2_MERGE;
            emu_deferred(Q.data(), R, p.Kf.data(), p.Vf.data(), T, KT, S, f, thr, out.data(), mo, lo);
            double rr = 0;
            for (int r = 0; r < R; ++r) rr = std::max(rr, ratio_vs_ref(&Qd[(size_t)r * HD], p, all, &out[(size_t)r * HD], true, true));
            // the partials: m_s + log2 l_s against the split's LSE, and max s - THR <= m_s <= max s
            const int ntt = (T + KT - 1) / KT;
            for (int r = 0; r < R; ++r)
              for (int s = 0; s < S; ++s) {
                const int b = s * ntt / S * KT, e = std::min(T, (s + 1) * ntt / S * KT);
                std::vector<long long> ks(all.begin() + b, all.begin() + e);
                Att a;
                attend(&Qd[(size_t)r * HD], HD, scale_log2(), p.Kd.data(), HD, p.Vd.data(), HD, HD, ks.data(), (int)ks.size(), HD, a);
                const double m = mo[(size_t)r * S + s], l = lo[(size_t)r * S + s];
                const double r1 = std::fabs(m + std::log2(l) - a.lse) / tol_lse(a.lse, a.ds, a.n);
                const double slack = 2 * a.ds + 2 * U24 * std::fabs(a.smax);
                const double r2 = (m <= a.smax + slack && m >= a.smax - thr - slack) ? 0.0 : 2.0;
                if (fault == F2_NONE) worst_inv = std::max(worst_inv, std::max(r1, r2));
                rr = std::max(rr, std::max(r1, r2));
              }
            if (fault == F2_NONE) {
              worst = std::max(worst, rr);
              EXPECT(rr <= 0.5, "deferred emulation cfg %s KT=%d S=%d ratio %.3f", mixed ? "mixed" : gen_name(cfg), KT, S, rr);
            } else if (cfg == PLAIN) {
              plain_ratio = std::max(plain_ratio, rr);
              plain_ok &= rr <= 1.0;
            } else if (rr > 1.0) rej = true;
          }
      }
      if (fault == F2_NONE) {
        std::printf("emulation: deferred-rescale tiles (32 / 64 keys), worst error/tolerance %.3f (partials %.3f)\n", worst, worst_inv);
        continue;
      }
      std::printf("defect: %s: forcing %s, plain %s (ratio %.2f)\n", name[fault], rej ? "rejected" : "ACCEPTED",
                  plain_ok ? "accepted" : "rejected", plain_ratio);
      EXPECT(rej, "defect not caught: %s", name[fault]);
      if (must_hide_on_plain[fault]) EXPECT(plain_ok, "defect visible on plain input (expected hidden): %s", name[fault]);
    }
  }

  // ---------------- a finished row stored: through the comparator attn_check uses (Image / compare).  Three rows, row 1
  // finished: its elements are outside the write set.  The faulty kernel stores it too, with the right VALUES.
  {
    bool rej = false, rej_plain = false, clean = true;
    for (int gen : {(int)PLAIN, (int)STAIRS}) {
      const Panel& p = gen == PLAIN ? plain : forcing;
      Image im(3 * HD);
      std::vector<uint8_t> good(3 * HD * 2), bad;
      fill_sentinel(good.data(), good.size());
      bad = good;
      for (int r = 0; r < 3; ++r) {
        float qf[HD], out[HD];
        double qd[HD];
        make_q(gen, 400 + r, qf, qd);
        emu_onepass(qf, p.Kf.data(), p.Vf.data(), cut(all, 4, true), {}, out);
        Att a;
        attend(qd, HD, scale_log2(), p.Kd.data(), HD, p.Vd.data(), HD, HD, all.data(), T, HD, a);
        for (int e = 0; e < HD; ++e) {
          const uint16_t v = f2b(out[e]);
          std::memcpy(&bad[(size_t)(r * HD + e) * 2], &v, 2);
          if (r == 1) continue;
          std::memcpy(&good[(size_t)(r * HD + e) * 2], &v, 2);
          im.ref[r * HD + e] = a.o[e];
          im.tol[r * HD + e] = tol_out(a.o[e], a.A[e], a.ds, a.n, false, a.vmax[e]);
        }
      }
      clean &= compare<uint16_t>(im, good).ok();
      const Cmp c = compare<uint16_t>(im, bad);
      (gen == PLAIN ? rej_plain : rej) = !c.ok() && c.sentinel_bad > 0;
    }
    std::printf("defect: a finished row stored: forcing %s, plain %s (the sentinel, on any input)\n", rej ? "rejected" : "ACCEPTED",
                rej_plain ? "rejected" : "ACCEPTED");
    EXPECT(clean, "comparator flags a correct image with a finished row");
    EXPECT(rej && rej_plain, "defect not caught: a finished row stored");
  }

  // ---------------- (c) layouts
  {
    for (int x = 0; x < 16; ++x) {
      const int y = xswap23(x);
      EXPECT(xswap23(y) == x && (y & 3) == (x & 3) && ((y >> 2) & 1) == ((x >> 3) & 1) && ((y >> 3) & 1) == ((x >> 2) & 1), "xswap23(%d)", x);
    }
    for (int d : {384, 512, 768, 1024, 1280}) {
      int qw, nw;
      xgeometry(d, qw, nw);
      EXPECT(qw * nw == d, "geometry d=%d", d);
      const int Tl = 77;     // 2 full tiles + 13 rows
      std::vector<char> seen((size_t)xslot_elems(Tl, d), 0);
      bool ok = true;
      for (int t = 0; t < Tl; ++t)
        for (int c = 0; c < d; ++c) {
          const long long i = xblocked_index(t, c, d);
          // direct formula: [tile][wave][32 rows][qw]
          const long long j = (long long)(t / 32) * 32 * d + (long long)(c / qw) * 32 * qw + (long long)(t % 32) * qw + c % qw;
          ok &= i == j && i >= 0 && i < (long long)seen.size() && !seen[(size_t)i];
          if (i >= 0 && i < (long long)seen.size()) seen[(size_t)i] = 1;
        }
      EXPECT(ok, "blocked-slot layout d=%d", d);
      const int H = d / 64, S = 3;
      const long long slab = 7;
      std::vector<char> su((size_t)S * H * d * slab, 0), sw((size_t)H * d * 64, 0), sk((size_t)H * d * 64, 0);
      bool oku = true, okw = true;
      for (int s = 0; s < S; ++s)
        for (int r = 0; r < slab; ++r)
          for (int h = 0; h < H; ++h)
            for (int c = 0; c < d; ++c) {
              const long long i = part_u_index(s, r, h, c, H, d, slab);
              oku &= i >= 0 && i < (long long)su.size() && !su[(size_t)i];
              if (i >= 0 && i < (long long)su.size()) su[(size_t)i] = 1;
              // a record holds 16 consecutive columns, bits 2 and 3 of the position swapped
              oku &= i / 16 == ((((long long)s * H + h) * (d / 16) + c / 16) * slab + r) && xswap23((int)(i % 16)) == c % 16;
            }
      for (int h = 0; h < H; ++h)
        for (int j = 0; j < 64; ++j)
          for (int c = 0; c < d; ++c) {
            const long long i = wvb_index(h, j, c, d), k = wkt_index(h, j, c, d);
            okw &= i >= 0 && i < (long long)sw.size() && !sw[(size_t)i] && k >= 0 && k < (long long)sk.size() && !sk[(size_t)k];
            if (i >= 0 && i < (long long)sw.size()) sw[(size_t)i] = 1;
            if (k >= 0 && k < (long long)sk.size()) sk[(size_t)k] = 1;
            // u record position p pairs with wvb position p of the same 16-column block
            okw &= i % 16 == part_u_index(0, 0, h, c, H, d, slab) % 16;
          }
      EXPECT(oku, "part_u layout d=%d", d);
      EXPECT(okw, "wvb / wkt layout d=%d", d);
      EXPECT(part_ml_index(2, 5, 3, H, slab) == 2 * ((2 * slab + 5) * H + 3), "part_ml layout");
    }
    for (int c = 0; c < 256; ++c) {
      if ((c & 0x7f) == 0x7f) continue;
      const double v = e4m3((uint8_t)c);
      EXPECT(std::fabs(v) <= 448.0 && (double)rb((float)v) == v, "e4m3 code %d is not an exact bf16", c);
    }
    EXPECT(e4m3(0x7e) == 448.0 && e4m3(0x38) == 1.0 && e4m3(0x01) == std::ldexp(1.0, -9) && e4m3(0xb8) == -1.0, "e4m3 decode");
    std::printf("layouts: blocked slot, xswap23, part_u / part_ml, wvb / wkt, e4m3 ok\n");
  }

  if (g_fail) { std::printf("selftest FAILED: %d\n", g_fail); return 1; }
  std::printf("selftest ok\n");
  return 0;
}
