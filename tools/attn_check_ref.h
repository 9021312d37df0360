// Host-only reference, input generators and comparator of tools/attn_check (no HIP in this file:
// tools/attn_check_selftest.cpp exercises it on the CPU).  All reference arithmetic is f64 on the same bf16 (or
// e4m3 x f32 scale) inputs the kernel gets.
//
// For one (row, head) over a key list the reference gives the scores s_t (log2 units), LSE = log2 sum_t 2^s_t,
// p_t = 2^(s_t - LSE), o_e = sum_t p_t v_te and A_e = sum_t p_t |v_te|.  The key list is what the kernel is given:
// self: positions 0..row_pos through lin[hyp][p]; cross: the slot's T keys; a split: that split's keys only.
//
// Tolerances are per element and built from reference quantities; every constant is a count of the kernel's rounding
// steps times a unit roundoff (U9 = 2^-9 for a bf16 rounding, U24 = 2^-24 for f32), doubled for margin.  Each count
// names the statement it comes from (attn_dec.hip = AD, attn_xenc.hip = AX; kernel :: statement):
//   score    ds_t = (n_fma + 1) U24 S_t, S_t = sum_i |q_i k_ti| scale.
//            n_fma = 64 for a head: AD self_attn_wave_kernel / cross_item / cross_capture_kernel / dec_attn_kernel ::
//              `d = fmaf(qf[i], bf2f(kr[u][i]), d)` x 8 and `d += __shfl_xor(d, 1 | 2 | 4)` (11 roundings on a chain,
//              counted as 64, any order); AD cross_tf_kernel :: `scores`: 4 x mfma_f32_32x32x16_bf16 = 64 products.
//            n_fma = d + NW for the factored form: AX xattn_segment :: `sc = mfma(ea, qf[s], sc)` over QW columns per
//              wave and `v += sX[(w2 * 16 + r) * 64 + lane]` over the NW waves.
//            + 1: `qf[i] *= a.scale_log2` (VALU), `sc[kb][e] * sl2` (cross_tf), `sc[4 g + e2] *= sv[e2]` (fp8 scale).
//            In any summation order (Higham, Accuracy and Stability, eq. 3.5).
//   p        relative error ln2 ds + 4 U24: `sc[u] - ms` (1), exp2f (2 ulp), `1.0f / l` and `o[i] * inv` (1, shared
//            with the output below)
//   kappa    2 (2 (ln2 ds + 4 U24) + n_acc U24): numerator and denominator both carry p's error (factor 2);
//            n_acc = n + n / 8 + 16: `x = fmaf(pu[u], bf2f(vr[u][i]), x)` / the U^T MFMA once per key (n, any order);
//              `o[i] * corr` / `o[c][r] *= alpha` at most once per chunk of >= 8 keys (n / 8); the merges
//              `o[r][i] * ca + oo * cb` x 3 lane-group steps, `O += s_o[w][r][e] * c` x 4 waves, and
//              `o += po[s] * w` in cross_combine_kernel / combine_l2 (<= 16 splits; counted 16 in all: a split
//              replaces, not adds to, the per-key chain it cuts)
//   out      bf16 output of an f32 kernel:      2 U9 |ref_e| + kappa A_e          (`f2bf(O / L)`, `f2bf(o[i] * inv)`)
//            kernels rounding P to bf16:       + 2 U9 A_e   (`pf[..] = f2bf(pv[e])` in cross_tf_kernel, `f2bf(F8 ?
//            p * ps[r] : p)` in xattn_segment: P rounded once, relative U9; l sums the unrounded p)
//            the factored chain:               + 2 U9 A_e   (xstore_u :: `f2bf(o[c][8 gp + e] * inv)`, the bf16
//            partial u_s / l_s; merged in xcomb_vo_kernel as bf16 hi + lo, `ul[i] = f2bf(u[i] - bf2f(uh[i]))`, which
//            leaves 2^-8 x 2^-8 of u: counted as u^2 = 2^-16, negligible beside the d U24 of the MFMA sum)
//            + n 2^-118 max_t |v_te| + 2^-126: f32 underflow.  A weight below 2^-126 of the running maximum is flushed
//            (or denormal); the running maximum lags the true one by at most 2^8 (the rescale threshold) and l >= 1,
//            so each of the n normalised weights is off by at most 2^-118 absolutely; the output's own floor is 2^-126
//   LSE      |m + log2 l - LSE| <= 2 (ds + (n_acc + 4) U24 / ln2 + |LSE| U24)   (`l_run += p` per key, the rescales
//            and merges of l as for o; m itself is an f32 score)
//   probs    |p - p_ref| <= 2 p_ref (ln2 ds + (n + 4) U24) + 2^-126 (`s_sc[p] * inv` / `pv[..] * inv_cap`: l's
//            accumulation over n keys; one f32 denormal floor), each row's sum within n U24 of 1
// U9 is half of bf16's true unit roundoff (8 significant bits: a store is off by up to 2^-8 |x|), so the doubled
// 2 U9 |ref| term is exactly one bf16 store and carries no margin: a faultless kernel reaches a ratio just below 1 on
// a well-conditioned element (0.995 seen), and that is not a near miss.  The margin is in the kappa terms.
// Generators: the levels are rounded to bf16 like every input.  Above 128 nats (256 for STAIRS) a level's spacing is
// 1 (2) nat, so late STAIRS steps are 6 or 8 nats (8.7 or 11.5 log2 units, still above the threshold of 8) and UNDER
// steps 4 or 5 nats (5.8 or 7.2; below it).  UNDER still rescales, every second tile: the running maximum lags by
// up to 2 steps, so P reaches 2^6..2^8 before its bf16 rounding, which is what it is for.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

namespace acr {

constexpr double U24 = 1.0 / 16777216.0, U9 = 1.0 / 512.0, LN2 = 0.69314718055994530942;
constexpr int HD = 64;
// the kernels' f32 scale constant (1/8 log2 e as attn_dec.hip / attn_xenc.hip form it), widened exactly
inline double scale_log2() { return (double)(0.125f * 1.4426950408889634f); }

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
inline float rb(float f) { return b2f(f2b(f)); }
// OCP e4m3 (bias 7, no inf, 0x7f = NaN) -> f64
inline double e4m3(uint8_t c) {
  const int s = c >> 7, e = (c >> 3) & 15, m = c & 7;
  const double v = e == 0 ? std::ldexp((double)m, -9) : std::ldexp(1.0 + m / 8.0, e - 7);
  return s ? -v : v;
}

// Sentinel byte at byte offset b of an output buffer (position dependent: a shifted copy does not pass)
inline uint8_t sentinel(size_t b) { return (uint8_t)(0xA0 + b % 89); }
inline void fill_sentinel(uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) p[i] = sentinel(i);
}
inline size_t guard_damage(const uint8_t* g, size_t n, uint8_t fill, size_t* first = nullptr) {
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i)
    if (g[i] != fill) {
      if (!bad && first) *first = i;
      ++bad;
    }
  return bad;
}

struct Rng {                              // splitmix64 + Box-Muller: the same stream on every host
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uni() { return ((next() >> 11) + 0.5) / 9007199254740992.0; }
  double randn() { return std::sqrt(-2.0 * std::log(uni())) * std::cos(6.283185307179586 * uni()); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

// ---------------------------------------------------------------------------------------------------------------
// Reference attention of one query over a key list.  K / V are f64 row arrays; keys[i] is the row index of key i.
struct Att {
  int n = 0;
  std::vector<double> s, sabs, p;         // per key: score (log2 units), sum |q k| scale, probability
  double smax = 0, lse = 0, ds = 0;       // ds: the largest score bound (n_fma + 1) U24 S_t over the keys (undoubled)
  std::vector<double> o, A, vmax;         // per output element (vmax = max_t |v_te|)
};
inline void attend(const double* q, int dk, double scale, const double* K, long long ldk, const double* V, long long ldv,
                   int dv, const long long* keys, int n, int n_fma, Att& r) {
  r.n = n;
  r.s.resize(n); r.sabs.resize(n); r.p.resize(n);
  r.o.assign(dv, 0.0); r.A.assign(dv, 0.0); r.vmax.assign(dv, 0.0);
  r.smax = -INFINITY; r.ds = 0;
  for (int t = 0; t < n; ++t) {
    const double* k = K + keys[t] * ldk;
    double a = 0, b = 0;
    for (int i = 0; i < dk; ++i) { const double x = q[i] * k[i]; a += x; b += std::fabs(x); }
    r.s[t] = a * scale; r.sabs[t] = b * std::fabs(scale);
    r.smax = std::max(r.smax, r.s[t]);
    r.ds = std::max(r.ds, (n_fma + 1) * U24 * r.sabs[t]);
  }
  double l = 0;
  for (int t = 0; t < n; ++t) l += std::exp2(r.s[t] - r.smax);
  r.lse = r.smax + std::log2(l);
  for (int t = 0; t < n; ++t) {
    r.p[t] = std::exp2(r.s[t] - r.lse);
    const double* v = V + keys[t] * ldv;
    for (int e = 0; e < dv; ++e) r.vmax[e] = std::max(r.vmax[e], std::fabs(v[e]));
    if (r.p[t] == 0.0) continue;
    for (int e = 0; e < dv; ++e) { r.o[e] += r.p[t] * v[e]; r.A[e] += r.p[t] * std::fabs(v[e]); }
  }
}

inline int n_acc(int n) { return n + n / 8 + 16; }
inline double kappa(double ds, int n) { return 2.0 * (2.0 * (LN2 * ds + 4 * U24) + n_acc(n) * U24); }
inline double tol_out(double ref, double A, double ds, int n, bool p_bf16, double vmax) {
  return 2 * U9 * std::fabs(ref) + (kappa(ds, n) + (p_bf16 ? 2 * U9 : 0.0)) * A + n * std::ldexp(vmax, -118) + std::ldexp(1.0, -126);
}
inline double tol_lse(double lse, double ds, int n) { return 2.0 * (ds + (n_acc(n) + 4) * U24 / LN2 + std::fabs(lse) * U24); }
inline double tol_prob(double p, double ds, int n) { return 2.0 * p * (LN2 * ds + (n + 4) * U24) + std::ldexp(1.0, -126); }

// Worst error / tolerance ratio of a checked quantity, and where
struct Worst {
  double ratio = 0;
  long long at = -1;
  void see(double err, double tol, long long i) {
    const double r = (err != err) ? INFINITY : (tol > 0 ? err / tol : (err > 0 ? INFINITY : 0));
    if (r > ratio || at < 0) { ratio = std::max(ratio, r); at = i; }
  }
  void merge(const Worst& o) { if (o.ratio > ratio || at < 0) { ratio = o.ratio; at = o.at; } }
  bool ok() const { return ratio <= 1.0; }
};

// ---------------------------------------------------------------------------------------------------------------
// Expected contents of an output buffer: per element (value, tolerance), or tol < 0 = not written (sentinel bytes)
struct Image {
  std::vector<double> ref, tol;
  explicit Image(size_t n) : ref(n, 0.0), tol(n, -1.0) {}
};
struct Cmp {
  Worst w;
  size_t sentinel_bad = 0;
  bool ok() const { return w.ok() && sentinel_bad == 0; }
  std::string str() const {
    return (sentinel_bad ? std::to_string(sentinel_bad) + " bytes outside the write set changed; " : std::string()) +
           "worst at element " + std::to_string(w.at);
  }
};
template <class T>
inline Cmp compare(const Image& im, const std::vector<uint8_t>& got) {
  Cmp c;
  for (size_t i = 0; i < im.ref.size(); ++i) {
    if (im.tol[i] < 0) {
      for (size_t b = i * sizeof(T); b < (i + 1) * sizeof(T); ++b) c.sentinel_bad += got[b] != sentinel(b);
      continue;
    }
    double v;
    if (sizeof(T) == 2) { uint16_t u; std::memcpy(&u, &got[i * 2], 2); v = b2f(u); }
    else { float f; std::memcpy(&f, &got[i * 4], 4); v = f; }
    c.w.see(std::fabs(v - im.ref[i]), im.tol[i], (long long)i);
  }
  return c;
}

// ---------------------------------------------------------------------------------------------------------------
// Input generators.  A key row carries six PROFILE channels (elements 0..5) and noise elsewhere; the query picks one
// channel with the value `QSEL`, so rows that share a K panel (a beam group, an m-tile) can follow different
// profiles.  level(t) below is in nats for the head form (score = 1/8 q.k) and every value is rounded to bf16 before
// use, so the reference sees exactly what the kernel sees.
enum Gen { PLAIN = 0, STAIRS, UNDER, FIRST, LAST, EDGES, OFF_NEG, OFF_POS, FLAT, N_GEN };
inline const char* gen_name(int g) {
  static const char* n[] = {"plain", "stairs", "under", "first", "last", "edges", "offset-", "offset+", "flat"};
  return n[g];
}
constexpr int N_CH = 6;                   // channels: 0 stairs, 1 under, 2 first, 3 last, 4 edges, 5 constant one
constexpr double NOISE = 0.39;            // 0.02 sqrt(384): the synthetic model's q / k / v element scale

// Profile level of key position t in nats.  thr = the deferred-rescale threshold in log2 units (attn.h).  `bounds`
// = first keys of the splits in use (EDGES puts a spike on the first and last key of every split, alternating 0 and
// 110 nats = 159 log2 units between neighbouring splits so that merge weights underflow to exactly 0).
inline double level(int ch, int t, int T, double thr, const std::vector<int>& bounds) {
  switch (ch) {
    case 0: return (t % 32 == 17) ? (thr + 1.4) * LN2 * (t / 32 + 1) : 0.0;      // +9.4 log2 per 32-key tile
    case 1: return (t % 32 == 17) ? (thr - 1.5) * LN2 * (t / 32 + 1) : 0.0;      // +6.5 log2 per tile: never rescales
    case 2: return t == 0 ? 20.0 : (t == T - 1 ? 19.0 : 0.0);
    case 3: return t == T - 1 ? 20.0 : 0.0;
    case 4:
      for (size_t j = 0; j < bounds.size(); ++j) {
        const int b0 = bounds[j], b1 = (j + 1 < bounds.size() ? bounds[j + 1] : T) - 1;
        if (t == b0 || t == b1) return (j & 1) ? 110.0 : 12.0;
      }
      return 0.0;
    default: return 1.0;
  }
}
// One key row and one value row of `dim` elements (bf16 bits).  sel = the value a selecting query holds (8 for the head
// form, where score = q.k / 8 in nats); the channel value is level / (sel / 8)... i.e. q[ch] k[ch] / 8 = level.
// Values: |noise| with a sign that depends on the element only, so A_e = |o_e| (the bound stays tight on spikes);
// `plain_v` gives signed noise instead.
inline void gen_key_row(Rng& g, int t, int T, double thr, const std::vector<int>& bounds, int dim, uint16_t* k) {
  for (int c = 0; c < dim; ++c) k[c] = c < N_CH ? f2b((float)level(c, t, T, thr, bounds)) : (c < 8 ? 0 : f2b((float)(g.randn() * NOISE)));
}
inline void gen_val_row(Rng& g, int dim, bool plain_v, uint16_t* v) {
  for (int c = 0; c < dim; ++c) {
    const double x = g.randn() * NOISE;
    v[c] = f2b((float)(plain_v ? x : ((c * 7 + 3) % 5 < 2 ? -1.0 : 1.0) * (std::fabs(x) + 0.05)));
  }
}
// A query of `dim` elements for generator gen.  unit = the query value that makes q[ch] k[ch] scale = level in the
// units the kernel's scale produces (head form: 8, since scale = 1/8 in nats; factored form: 1 / ln2 for log2 units).
inline void gen_query(Rng& g, int gen, int dim, double unit, uint16_t* q, double qnoise = NOISE) {
  for (int c = 0; c < dim; ++c) q[c] = c < 8 ? 0 : f2b((float)(g.randn() * qnoise));
  switch (gen) {
    case PLAIN: break;
    case STAIRS: q[0] = f2b((float)unit); break;
    case UNDER: q[1] = f2b((float)unit); break;
    case FIRST: q[2] = f2b((float)unit); break;
    case LAST: q[3] = f2b((float)unit); break;
    case EDGES: q[4] = f2b((float)unit); break;
    case OFF_NEG: q[5] = f2b((float)(-83.0 * unit)); q[0] = f2b((float)unit); break;   // -120 log2 units + stairs
    case OFF_POS: q[5] = f2b((float)(83.0 * unit)); q[1] = f2b((float)unit); break;    // +120 log2 units + under
    default: for (int c = 0; c < dim; ++c) q[c] = 0; break;                            // FLAT: every score 0
  }
}
// MIXED: row i of a tile takes generator mixed_gen(i): all of them in turn, FLAT included
inline int mixed_gen(int i) { return (i * 5 + 1) % N_GEN; }

// ---------------------------------------------------------------------------------------------------------------
// Layouts of the factored form (attn_xenc.hip), as direct index formulas
inline int xswap23(int x) { return (x & 3) | ((x >> 1) & 4) | ((x << 1) & 8); }
inline void xgeometry(int d, int& qw, int& nw) {
  switch (d) {
    case 384: qw = 96; nw = 4; return;
    case 512: qw = 64; nw = 8; return;
    case 768: qw = 96; nw = 8; return;
    case 1024: qw = 128; nw = 8; return;
    default: qw = 160; nw = 8; return;
  }
}
inline long long xslot_elems(int T, int d) { return (long long)((T + 31) / 32) * 32 * d; }
// element (t, c) of a window inside its tile-blocked slot [tile][wave][32][QW]
inline long long xblocked_index(int t, int c, int d) {
  int qw, nw;
  xgeometry(d, qw, nw);
  return (((long long)(t / 32) * nw + c / qw) * 32 + t % 32) * qw + c % qw;
}
// part_u [splits][H][d/16][slab_rows][16]: column c of (split, row, head) sits at position xswap23(c % 16) of its record
inline long long part_u_index(int split, int row, int h, int c, int H, int d, long long slab_rows) {
  return ((((long long)split * H + h) * (d / 16) + c / 16) * slab_rows + row) * 16 + xswap23(c % 16);
}
// part_ml [splits][slab_rows][H][2]
inline long long part_ml_index(int split, int row, int h, int H, long long slab_rows) {
  return 2 * (((long long)split * slab_rows + row) * H + h);
}
// wvb [H][d/16][64][16] = Wv[h*64 + j][16 (c/16) + xswap23(p)]; wkt [H][d][64] = Wk[h*64 + j][c]
inline long long wvb_index(int h, int j, int c, int d) { return (((long long)h * (d / 16) + c / 16) * 64 + j) * 16 + xswap23(c % 16); }
inline long long wkt_index(int h, int j, int c, int d) { return ((long long)h * d + c) * 64 + j; }

// run f(i) for i in [0, n) on up to 16 threads
inline void parallel_for(int n, const std::function<void(int)>& f) {
  const int nt = (int)std::max(1u, std::min(16u, std::min(std::thread::hardware_concurrency(), (unsigned)n)));
  if (nt <= 1) { for (int i = 0; i < n; ++i) f(i); return; }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] { for (int i = t; i < n; i += nt) f(i); });
  for (auto& t : th) t.join();
}

}  // namespace acr
