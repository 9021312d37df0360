// Isolated conformance check of the decoder attention kernels (vlog_amd/csrc/attn_dec.hip, attn_xenc.hip): every
// launcher of attn.h alone, no engine, no model, no weight files, against the f64 reference of tools/attn_check_ref.h
// on the same bf16 inputs, with per-element tolerances counted from the kernels' rounding steps (see that header).
// Inputs are the forcing generators of the header (stairs / under / first / last / edges / offsets / flat, mixed over
// the rows of one wave or m-tile) at T = 1500, n_ctx = 448: they drive the deferred-rescale branches mid-stream, put
// the row maximum in the ragged last tile, and make split maxima differ until merge weights underflow, so a dropped or
// doubled key, a wrong rescale or a wrong merge weight changes the output by far more than any bound.
// Every buffer sits between 0xFF guards; outputs, probabilities and scratch are prefilled with a position-dependent
// sentinel and every byte outside the reference's write set must be unchanged; counters must read zero after a launch.
//
// Usage: attn_check self|cross_group|cross_capture|cross_tf|xq|xattn|xcomb|xchain|all [-v]
// One line per non-passing case, then `family <name>: ok|FAIL`.  Exit 0 ok, 1 mismatch, 2 HIP error (at once).
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <map>
#include <string>

#include "../vlog_amd/csrc/attn.h"
#include "attn_check_ref.h"

using namespace acr;

static bool g_verbose = false;
static double g_ref_seconds = 0;

#define CK(x)                                                                         \
  do {                                                                                \
    hipError_t e__ = (x);                                                             \
    if (e__ != hipSuccess) {                                                          \
      std::printf("HIP error: %s: %s\n", #x, hipGetErrorString(e__));                 \
      std::fflush(stdout);                                                            \
      _exit(2);                                                                       \
    }                                                                                 \
  } while (0)

// a launcher call: an exception here is a failed launch (WM_LAUNCH_CHECK) -> status 2, nothing more is launched
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
// a call that must be refused by the launcher's own validation (before any launch)
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

struct Timer {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  ~Timer() { g_ref_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

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
  void zero_fill(size_t n) {
    alloc(n);
    CK(hipMemset(raw + GUARD, 0, n));
  }
  template <class T> T* p() const { return (T*)(raw + GUARD); }
  std::vector<uint8_t> get() const {
    std::vector<uint8_t> v(bytes);
    CK(hipMemcpy(v.data(), raw + GUARD, bytes, hipMemcpyDeviceToHost));
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
  int fails = 0, cases = 0, loose = 0;
  double worst = 0;
  std::string worst_case;
  void result(const std::string& cs, bool ok, double ratio, const std::string& detail = "") {
    ++cases;
    if (ratio > worst) { worst = ratio; worst_case = cs; }
    if (!ok) ++fails;
    if (!ok || g_verbose)
      std::printf("  %s %s %s ratio %.3f %s\n", ok ? "ok  " : "FAIL", name.c_str(), cs.c_str(), ratio, detail.c_str());
  }
  void guards(const std::string& cs, std::initializer_list<const DBuf*> bufs) {
    size_t bad = 0;
    for (const DBuf* b : bufs)
      if (b->raw) bad += b->guards_bad();
    if (bad) result(cs + " guards", false, INFINITY, std::to_string(bad) + " guard bytes changed");
  }
  int finish() {
    std::printf("family %s: %s (%d cases, worst error/tolerance %.3f at %s)\n", name.c_str(), fails ? "FAIL" : "ok", cases, worst,
                worst_case.c_str());
    std::fflush(stdout);
    return fails ? 1 : 0;
  }
};

static bool all_zero(const std::vector<uint8_t>& v) {
  for (uint8_t b : v) if (b) return false;
  return true;
}

static const double THR_TF = CROSS_TF_RESCALE_THR, THR_X = XATTN_RESCALE_THR;
static const int T_ENC = 1500, N_CTX = 448;

// ==================================================================================================================
// self: launch_self_attn
static int fam_self() {
  Fam F{"self"};
  const int H = 6, d = H * HD, NC = N_CTX, NHYP = 48, PMAX = 45;
  static const int POS1[17] = {1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 447, 448};
  std::vector<uint16_t> kc((size_t)NHYP * H * NC * HD), vc(kc.size());
  {
    Rng g(1);
    const std::vector<int> bounds = {0, 112, 224, 336};
    for (int hyp = 0; hyp < NHYP; ++hyp)
      for (int h = 0; h < H; ++h)
        for (int p = 0; p < NC; ++p) {
          const size_t o = (((size_t)hyp * H + h) * NC + p) * HD;
          gen_key_row(g, p, NC, THR_TF, bounds, HD, &kc[o]);
          gen_val_row(g, HD, hyp % 4 == 0, &vc[o]);
        }
  }
  std::vector<int> lin((size_t)NHYP * NC), done(NHYP), row_hyp(PMAX), row_pos(PMAX);
  for (int hyp = 0; hyp < NHYP; ++hyp) {
    done[hyp] = hyp % 3 == 1;
    for (int p = 0; p < NC; ++p) lin[(size_t)hyp * NC + p] = (hyp + 1 + p * 5) % NHYP;   // a different slot per position
  }
  for (int r = 0; r < PMAX; ++r) {
    row_hyp[r] = (r * 7 + 3) % NHYP;
    row_pos[r] = POS1[(r * 5 + 2) % 17] - 1;
  }
  // q rows inside a qkv row (ldq = 3 d) and packed (ldq = d): the same q values in both
  std::vector<uint16_t> q3((size_t)PMAX * 3 * d), q1((size_t)PMAX * d);
  {
    Rng g(2);
    for (auto& x : q3) x = f2b((float)g.randn());
    for (int r = 0; r < PMAX; ++r)
      for (int h = 0; h < H; ++h) {
        gen_query(g, mixed_gen(r + h), HD, 8.0, &q3[(size_t)r * 3 * d + h * HD]);
        std::memcpy(&q1[(size_t)r * d + h * HD], &q3[(size_t)r * 3 * d + h * HD], HD * 2);
      }
  }
  DBuf dk, dv, dlin, ddone, drh, drp, dq3, dq1, dout;
  dk.put(kc); dv.put(vc); dlin.put(lin); ddone.put(done); drh.put(row_hyp); drp.put(row_pos); dq3.put(q3); dq1.put(q1);

  // references of all PMAX rows, with the lineage table and with identity
  std::vector<Att> ref[2];
  {
    Timer tm;
    for (int wl = 0; wl < 2; ++wl) {
      ref[wl].resize((size_t)PMAX * H);
      parallel_for(PMAX * H, [&](int i) {
        const int r = i / H, h = i % H, hyp = row_hyp[r], nk = row_pos[r] + 1;
        std::vector<double> K((size_t)nk * HD), V((size_t)nk * HD), q(HD);
        std::vector<long long> keys(nk);
        for (int p = 0; p < nk; ++p) {
          const int ph = wl ? lin[(size_t)hyp * NC + p] : hyp;
          const size_t o = (((size_t)ph * H + h) * NC + p) * HD;
          for (int e = 0; e < HD; ++e) { K[(size_t)p * HD + e] = b2f(kc[o + e]); V[(size_t)p * HD + e] = b2f(vc[o + e]); }
          keys[p] = p;
        }
        for (int e = 0; e < HD; ++e) q[e] = b2f(q1[(size_t)r * d + h * HD + e]);
        attend(q.data(), HD, scale_log2(), K.data(), HD, V.data(), HD, HD, keys.data(), nk, HD, ref[wl][i]);
      });
    }
  }
  const int ldo = d, OROWS = PMAX + 2;
  auto image = [&](int r0, int r1, int wl, bool wd) {
    Image im((size_t)OROWS * ldo);
    for (int r = r0; r < r1; ++r) {
      if (wd && done[row_hyp[r]]) continue;
      for (int h = 0; h < H; ++h) {
        const Att& a = ref[wl][(size_t)r * H + h];
        for (int e = 0; e < HD; ++e) {
          const size_t i = (size_t)r * ldo + h * HD + e;
          im.ref[i] = a.o[e];
          im.tol[i] = tol_out(a.o[e], a.A[e], a.ds, a.n, false, a.vmax[e]);
        }
      }
    }
    return im;
  };
  // rows [r0, r1) of a pass of `plan` rows, written at their own rows of a sentinel-filled out buffer
  auto run = [&](int r0, int r1, int plan, int group, int wl, bool wd, bool l3) {
    dout.sentinel_fill((size_t)OROWS * ldo * 2);
    const long long ldq = l3 ? 3 * d : d;
    const uint16_t* qb = l3 ? dq3.p<uint16_t>() : dq1.p<uint16_t>();
    launch("launch_self_attn", [&] {
      launch_self_attn((const bf16*)(qb + (size_t)r0 * ldq), ldq, dk.p<bf16>(), dv.p<bf16>(), wl ? dlin.p<int>() : nullptr,
                       drh.p<int>() + r0, drp.p<int>() + r0, wd ? ddone.p<int>() : nullptr, dout.p<bf16>() + (size_t)r0 * ldo, ldo,
                       r1 - r0, H, NC, nullptr, nullptr, nullptr, nullptr, plan, group);
    });
    return dout.get();
  };
  std::map<std::string, std::vector<uint8_t>> whole;
  for (int P : {1, 5, 42, 43, 45})
    for (int wl = 0; wl < 2; ++wl)
      for (int wd = 0; wd < 2; ++wd)
        for (int l3 = 0; l3 < 2; ++l3) {
          const std::string cs = "rows " + std::to_string(P) + (wl ? " lineage" : " identity") + (wd ? " done" : "") + (l3 ? " ldq=3d" : " ldq=d");
          const auto got = run(0, P, P, 1, wl, wd, l3);
          const Cmp c = compare<uint16_t>(image(0, P, wl, wd), got);
          F.result(cs, c.ok(), c.w.ratio, c.str());
          F.guards(cs, {&dk, &dv, &dlin, &ddone, &drh, &drp, &dq3, &dq1, &dout});
          if (P % 5 == 0) {      // the XCD-remapped beam-group pair order gives the same bits
            const auto g5 = run(0, P, P, 5, wl, wd, l3);
            F.result(cs + " group 5 == group 1", g5 == got, g5 == got ? 0 : INFINITY);
          }
          if (wl && wd && l3) whole[std::to_string(P)] = got;
        }
  // a slice of a larger pass gives the bits of the whole pass's rows (plan_rows > rows), on both routes
  struct Slice { int P, r0, r1; };
  for (const Slice s : {Slice{45, 10, 30}, Slice{45, 40, 45}, Slice{42, 3, 8}, Slice{42, 41, 42}}) {
    const auto got = run(s.r0, s.r1, s.P, 1, 1, true, true);
    const auto& w = whole[std::to_string(s.P)];
    bool same = true;
    size_t outside = 0;
    for (size_t b = 0; b < got.size(); ++b) {
      const int r = (int)(b / ((size_t)ldo * 2));
      if (r >= s.r0 && r < s.r1) same &= got[b] == w[b];
      else outside += got[b] != sentinel(b);
    }
    F.result("slice [" + std::to_string(s.r0) + "," + std::to_string(s.r1) + ") of " + std::to_string(s.P) + " rows", same && !outside,
             same && !outside ? 0 : INFINITY, outside ? "bytes outside the slice changed" : "");
  }
  return F.finish();
}

// ==================================================================================================================
// The cross-attention launcher over projected K / V panels: one environment (panels, references) per head count
struct CrossEnv {
  int H = 0, NS = 0, T = T_ENC;
  std::vector<uint16_t> K, V;            // [slot][H][T][64]
  std::vector<double> Kd, Vd;
  DBuf dK, dV;
  void make(int H_, int NS_, const std::vector<int>& bounds, uint64_t seed) {
    H = H_; NS = NS_;
    K.resize((size_t)NS * H * T * HD); V.resize(K.size()); Kd.resize(K.size()); Vd.resize(K.size());
    Rng g(seed);
    for (int s = 0; s < NS; ++s)
      for (int h = 0; h < H; ++h)
        for (int t = 0; t < T; ++t) {
          const size_t o = (((size_t)s * H + h) * T + t) * HD;
          gen_key_row(g, t, T, THR_TF, bounds, HD, &K[o]);
          gen_val_row(g, HD, s == 0, &V[o]);
        }
    for (size_t i = 0; i < K.size(); ++i) { Kd[i] = b2f(K[i]); Vd[i] = b2f(V[i]); }
    dK.put(K); dV.put(V);
  }
};

struct CrossCfg {
  int rows = 1, group = 1, plan_rows = 0, cap = 0;
  bool cnt = false;                      // fz.cnt / fz.tf_cnt: in-kernel combine
  int slabs = 0;                         // q = bf16(sum of this many split-K slabs + bias) ...
  bool fuse = true;                      // ... summed by the kernel (fz.q_part), else on the host only
  int done = 0;                          // 0 no table, 1 a third of the hypotheses, 2 + the whole first group
  bool probs = false;
  int tf = 0, mfma = 0;
  bool slot_null = false;                // teacher-forced form without a slot table: row_hyp = the window index
  int launches = 1;                      // back to back on the same counters
  int gen_shift = 0;
  bool check = true;                     // compare with the f64 reference (else: only returned for a memcmp)
  bool partials = false;                 // check the (m, l, o) partials through the LSE form (splits > 1, no cnt)
};
struct CrossRes {
  std::vector<uint8_t> out, probs;
};

static int cross_splits(const CrossCfg& c, int H, int T, bool& use_tf) {
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

static CrossRes run_cross(Fam& F, CrossEnv& E, const CrossCfg& c, const std::string& cs) {
  const int H = E.H, T = E.T, d = H * HD, rows = c.rows, group = c.group;
  static const int HEAD_MAP6[6] = {0, -1, 1, -1, -1, 2};
  const int n_align = 4;                 // slot 3 belongs to no head: never written
  std::vector<int> head_map(H, -1);
  for (int h = 0; h < H; ++h) head_map[h] = h < 6 ? HEAD_MAP6[h] : -1;
  const int n_grp = (rows + group - 1) / group;
  const int n_hyp = c.slot_null ? n_grp : rows;
  std::vector<int> row_hyp(rows), hyp_slot(n_hyp), done(n_hyp, 0);
  for (int r = 0; r < rows; ++r) row_hyp[r] = c.slot_null ? r / group : rows - 1 - r;   // non-identity, groups contiguous
  for (int hy = 0; hy < n_hyp; ++hy) {
    const int g = c.slot_null ? hy : (rows - 1 - hy) / group;
    hyp_slot[hy] = c.slot_null ? hy : (g * 3 + 1) % E.NS;
    if (c.done >= 1) done[hy] = c.slot_null ? (n_grp > 1 && hy == 0) : hy % 3 == 1;
  }
  if (c.done >= 2)
    for (int r = 0; r < std::min(group, rows); ++r) done[row_hyp[r]] = 1;
  auto row_slot = [&](int r) { return c.slot_null ? row_hyp[r - r % group] : hyp_slot[row_hyp[r - r % group]]; };
  auto row_done = [&](int r) { return c.done && done[row_hyp[r]]; };

  // q: generator rows; with slabs, q = bf16(sum of the slabs in order + bias) formed on the host
  std::vector<uint16_t> q((size_t)rows * d);
  std::vector<float> slab, bias;
  const int q_rows = rows + 1;
  {
    Rng g(1000 + rows * 31 + group + c.gen_shift);
    for (int r = 0; r < rows; ++r)
      for (int h = 0; h < H; ++h) gen_query(g, mixed_gen(r + h + c.gen_shift), HD, 8.0, &q[(size_t)r * d + h * HD]);
    if (c.slabs) {
      slab.assign((size_t)c.slabs * q_rows * d, 0.f);
      bias.resize(d);
      for (int i = 0; i < d; ++i) bias[i] = i % HD < 8 ? 0.f : (float)(g.randn() * 0.1);
      for (int r = 0; r < rows; ++r)
        for (int i = 0; i < d; ++i) {
          float v = 0.f;
          for (int s = 0; s < c.slabs; ++s) {
            // the profile channels travel exactly in slab 0; the noise is spread over the slabs
            const float x = i % HD < 8 ? (s == 0 ? b2f(q[(size_t)r * d + i]) : 0.f) : (float)(g.randn() * NOISE / std::sqrt((double)c.slabs));
            slab[((size_t)s * q_rows + r) * d + i] = x;
            v += x;
          }
          q[(size_t)r * d + i] = f2b(v + bias[i]);
        }
    }
  }
  bool use_tf = false;
  const int splits = cross_splits(c, H, T, use_tf);
  DBuf dq, dslab, dbias, drh, dhs, ddone, dhm, dout, dprobs, dpm, dpl, dpo, dcnt;
  dq.put(q); drh.put(row_hyp); dhs.put(hyp_slot); ddone.put(done); dhm.put(head_map);
  if (c.slabs) { dslab.put(slab); dbias.put(bias); }
  const int OROWS = rows + 2;
  const size_t np = (size_t)rows * H * 16;
  dpm.sentinel_fill(np * 4); dpl.sentinel_fill(np * 4); dpo.sentinel_fill(np * HD * 4);
  dcnt.zero_fill((size_t)rows * H * 4);
  CrossFuse fz;
  if (c.slabs && c.fuse) { fz.q_part = dslab.p<float>(); fz.q_splits = c.slabs; fz.q_rows = q_rows; fz.q_bias = dbias.p<float>(); }
  fz.tf = c.tf; fz.mfma = c.mfma;
  if (c.cnt) { fz.cnt = dcnt.p<int>(); fz.tf_cnt = dcnt.p<int>(); }
  CrossRes res;
  for (int it = 0; it < c.launches; ++it) {
    dout.sentinel_fill((size_t)OROWS * d * 2);
    if (c.probs) dprobs.sentinel_fill((size_t)OROWS * n_align * T * 4);
    launch("launch_cross_attn", [&] {
      launch_cross_attn(c.slabs && c.fuse ? nullptr : dq.p<bf16>(), d, E.dK.p<bf16>(), E.dV.p<bf16>(), T, c.slot_null ? nullptr : dhs.p<int>(),
                        drh.p<int>(), c.done ? ddone.p<int>() : nullptr, dout.p<bf16>(), d, rows, H, group, dpm.p<float>(),
                        dpl.p<float>(), dpo.p<float>(), c.probs ? dprobs.p<float>() : nullptr, c.probs ? dhm.p<int>() : nullptr,
                        n_align, c.plan_rows, c.cap, fz, nullptr, nullptr, nullptr, nullptr);
    });
    const auto cn = dcnt.get();
    if (!all_zero(cn)) F.result(cs + " counters", false, INFINITY, "cnt words not zero after the launch");
    const auto got = dout.get();
    if (it > 0 && got != res.out) F.result(cs + " relaunch", false, INFINITY, "second launch on the same counters differs");
    res.out = got;
  }
  if (c.probs) res.probs = dprobs.get();
  F.guards(cs, {&dq, &dslab, &dbias, &drh, &dhs, &ddone, &dhm, &dout, &dprobs, &dpm, &dpl, &dpo, &dcnt, &E.dK, &E.dV});
  const auto pm = dpm.get(), pl = dpl.get(), po = dpo.get();
  {
    // the split scratch: only the records [(row H + h) splits + s], s < splits, of LIVE rows are written (none at one
    // split); every other byte keeps its sentinel, in every call
    Image im_m(np), im_o(np * HD);
    if (splits > 1)
      for (int r = 0; r < rows; ++r) {
        if (row_done(r)) continue;
        for (int h = 0; h < H; ++h)
          for (int s2 = 0; s2 < splits; ++s2) {
            const size_t pi = ((size_t)r * H + h) * splits + s2;
            im_m.tol[pi] = INFINITY;                       // written: checked through the LSE form where asked
            for (int x = 0; x < HD; ++x) im_o.tol[pi * HD + x] = INFINITY;
          }
      }
    const size_t bad = compare<float>(im_m, pm).sentinel_bad + compare<float>(im_m, pl).sentinel_bad + compare<float>(im_o, po).sentinel_bad;
    F.result(cs + " split scratch outside the write set", bad == 0, bad ? INFINITY : 0, std::to_string(bad) + " bytes changed");
  }
  if (!c.check) return res;

  // ---- reference
  std::vector<Att> ref((size_t)rows * H);
  std::vector<long long> all(T);
  for (int t = 0; t < T; ++t) all[t] = t;
  auto qd = [&](int r, int h, double* o) { for (int e = 0; e < HD; ++e) o[e] = b2f(q[(size_t)r * d + h * HD + e]); };
  {
    Timer tm;
    parallel_for(rows * H, [&](int i) {
      const int r = i / H, h = i % H;
      double qv[HD];
      qd(r, h, qv);
      const size_t o = ((size_t)row_slot(r) * H + h) * T * HD;
      attend(qv, HD, scale_log2(), &E.Kd[o], HD, &E.Vd[o], HD, HD, all.data(), T, HD, ref[i]);
    });
  }
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
  const Cmp co = compare<uint16_t>(im, res.out);
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
          std::memcpy(&f, &res.probs[i * 4], 4);
          sum += f;
        }
        worst_sum = std::max(worst_sum, std::fabs(sum - 1.0) / (T * U24));
      }
    }
    const Cmp cp = compare<float>(ip, res.probs);
    F.result(cs + " probs", cp.ok(), cp.w.ratio, cp.str());
    F.result(cs + " probs row sums", worst_sum <= 1.0, worst_sum);
  }
  if (c.partials && splits > 1 && !c.cnt) {
    // unnormalised f32 partials: m_s + log2 l_s against the split's LSE, o_s / l_s against its normalised output, and
    // (matrix-core kernel, deferred rescale) max s - THR <= m_s <= max s.  A row's partial record is
    // [(row H + h) splits + split]
    Timer tm;
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
        std::memcpy(&m, &pm[pi * 4], 4);
        std::memcpy(&l, &pl[pi * 4], 4);
        ws[i].see(std::fabs((double)m + std::log2((double)l) - a.lse), tol_lse(a.lse, a.ds, a.n), (long long)pi);
        const double slack = 2 * a.ds + 2 * U24 * std::fabs(a.smax);
        if (!(m <= a.smax + slack && m >= a.smax - (use_tf ? THR_TF : 0.0) - slack)) ws[i].see(INFINITY, 1, (long long)pi);
        for (int x = 0; x < HD; ++x) {
          float ov;
          std::memcpy(&ov, &po[(pi * HD + x) * 4], 4);
          // (f32 partial: only the arithmetic terms of the bound, no bf16 store)
          const double tol = tol_out(0.0, a.A[x], a.ds, a.n, use_tf, a.vmax[x]);
          ws[i].see(std::fabs((double)ov / (double)l - a.o[x]), tol, (long long)(pi * HD + x));
        }
      }
    });
    Worst w;
    for (auto& x : ws) if (x.at >= 0) w.merge(x);
    F.result(cs + " partials (LSE form)", w.ok(), w.ratio, "worst at record " + std::to_string(w.at));
  }
  return res;
}

static std::vector<int> group_bounds() {
  std::vector<int> b;
  for (int s = 0; s < 12; ++s) b.push_back(125 * s);
  return b;
}

static int fam_cross_group() {
  Fam F{"cross_group"};
  CrossEnv E;
  E.make(6, 4, group_bounds(), 7);
  struct RG { int rows, group; };
  int k = 0;
  for (const RG rg : {RG{9, 1}, RG{4, 2}, RG{6, 3}, RG{8, 4}, RG{10, 5}, RG{12, 6}, RG{7, 7}, RG{16, 16}}) {
    int rgc = 1;
    for (int c8 = 8; c8 >= 1; --c8)
      if (rg.group % c8 == 0 && rg.rows % c8 == 0) { rgc = c8; break; }
    for (int plan : {0, rgc == 1 ? 400 : 60 * rgc, 4000 * rgc}) {     // splits 12, a middle value (5 at RG 1, else 6), 1
      CrossCfg c;
      c.rows = rg.rows; c.group = rg.group; c.plan_rows = plan; c.gen_shift = k++;
      const std::string cs = "rows " + std::to_string(rg.rows) + " group " + std::to_string(rg.group) + " plan " + std::to_string(plan);
      c.partials = true;
      const CrossRes base = run_cross(F, E, c, cs);
      c.partials = false; c.check = false;
      auto same = [&](const char* what, const CrossCfg& v) {
        const CrossRes r = run_cross(F, E, v, cs + " " + what);
        F.result(cs + " " + what + " == base", r.out == base.out, r.out == base.out ? 0 : INFINITY);
      };
      { CrossCfg v = c; v.cap = 3; same("cap 3", v); }
      { CrossCfg v = c; v.cnt = true; v.launches = 2; same("in-kernel combine x2", v); }
      { CrossCfg v = c; v.cnt = true; v.cap = 5; same("in-kernel combine cap 5", v); }
      // partly and wholly finished groups, both combine forms
      for (int dn : {1, 2})
        for (int cn = 0; cn < 2; ++cn) {
          CrossCfg v = c;
          v.check = true; v.done = dn; v.cnt = cn; v.launches = cn ? 2 : 1;
          run_cross(F, E, v, cs + (dn == 2 ? " done+group" : " done") + (cn ? " cnt" : ""));
        }
    }
    // the fused q-slab load: the bits of the unfused call on the host-summed bf16 q (same slab order)
    for (int slabs : {1, 4, 16}) {
      CrossCfg c;
      c.rows = rg.rows; c.group = rg.group; c.slabs = slabs; c.gen_shift = k++;
      const std::string cs = "rows " + std::to_string(rg.rows) + " group " + std::to_string(rg.group) + " slabs " + std::to_string(slabs);
      const CrossRes fused = run_cross(F, E, c, cs);
      CrossCfg u = c;
      u.fuse = false; u.check = false;
      const CrossRes unf = run_cross(F, E, u, cs + " unfused");
      F.result(cs + " fused == unfused", fused.out == unf.out, fused.out == unf.out ? 0 : INFINITY);
    }
  }
  {
    DBuf dq;
    dq.zero_fill(64);
    CrossFuse fz;
    fz.q_part = dq.p<float>(); fz.q_splits = 17; fz.q_rows = 4; fz.q_bias = dq.p<float>();
    const bool th = throws([&] {
      launch_cross_attn(nullptr, 384, E.dK.p<bf16>(), E.dV.p<bf16>(), T_ENC, dq.p<int>(), dq.p<int>(), nullptr, dq.p<bf16>(), 384, 4, 6, 2,
                        nullptr, nullptr, nullptr, nullptr, nullptr, 0, 4, 0, fz, nullptr, nullptr, nullptr, nullptr);
    });
    F.result("17 slabs refused", th, th ? 0 : INFINITY);
  }
  return F.finish();
}

static std::vector<int> tf_bounds() {
  std::vector<int> b;
  for (int s = 0; s < 16; ++s) b.push_back(s * 24 / 16 * 64);
  return b;
}

static int fam_cross_capture() {
  Fam F{"cross_capture"};
  CrossEnv E;
  E.make(6, 4, group_bounds(), 8);
  struct RG { int rows, group; };
  int k = 0;
  // group 1: dec_attn_kernel<false>; 5, 8, 9, 17: cross_capture_kernel<8> (17: three blocks per group, the last with one row)
  for (const RG rg : {RG{9, 1}, RG{10, 5}, RG{16, 8}, RG{18, 9}, RG{34, 17}}) {
    CrossCfg c;
    c.rows = rg.rows; c.group = rg.group; c.probs = true; c.gen_shift = k++;
    run_cross(F, E, c, "rows " + std::to_string(rg.rows) + " group " + std::to_string(rg.group));
    // liveness is per row in both kernels: partly finished groups (also a block whose FIRST row is finished and whose
    // other rows are live), then a wholly finished first group
    for (int dn : {1, 2}) {
      CrossCfg v = c;
      v.done = dn; v.gen_shift = k++;
      run_cross(F, E, v, "rows " + std::to_string(rg.rows) + " group " + std::to_string(rg.group) + (dn == 2 ? " done+group" : " done"));
    }
  }
  {
    DBuf z;
    z.zero_fill(4096);
    CrossFuse fz;
    const bool th = throws([&] {
      launch_cross_attn(z.p<bf16>(), 384, E.dK.p<bf16>(), E.dV.p<bf16>(), 1537, z.p<int>(), z.p<int>(), nullptr, z.p<bf16>(), 384, 1, 6, 1,
                        nullptr, nullptr, nullptr, z.p<float>(), z.p<int>(), 1, 1, 0, fz, nullptr, nullptr, nullptr, nullptr);
    });
    F.result("T = 1537 refused", th, th ? 0 : INFINITY);
  }
  return F.finish();
}

static int fam_cross_tf() {
  Fam F{"cross_tf"};
  CrossEnv E;
  E.make(6, 2, tf_bounds(), 9);
  int k = 0;
  // teacher-forced: two windows; captured heads (two passes, exact max) and uncaptured ones (deferred rescale) in one launch
  for (int group : {16, 33, 128, 129, 150, 220})
    for (int sn = 0; sn < 2; ++sn)
      for (int dn = 0; dn < 2; ++dn) {
        if (dn && group != 33 && group != 129) continue;
        CrossCfg c;
        c.rows = 2 * group; c.group = group; c.tf = 1; c.probs = true; c.slot_null = sn; c.done = dn; c.gen_shift = k++;
        run_cross(F, E, c, "tf group " + std::to_string(group) + (sn ? " no slot table" : " slot table") + (dn ? " done" : ""));
      }
  // decode form: key splits 16 and 1 at H = 6, 13 at H = 20 (one window: 20 blocks)
  CrossEnv E20;
  E20.make(20, 1, tf_bounds(), 10);
  for (int group : {2, 5, 32})
    for (int mode = 0; mode < 3; ++mode) {
      CrossEnv& Ev = mode == 2 ? E20 : E;
      CrossCfg c;
      c.group = group; c.mfma = 1; c.gen_shift = k++;
      c.rows = mode == 2 ? group : 2 * group;
      c.plan_rows = mode == 1 ? 43 * group : 0;
      c.partials = true;
      const std::string cs = "decode group " + std::to_string(group) + (mode == 0 ? " splits 16" : mode == 1 ? " splits 1" : " splits 13");
      const CrossRes base = run_cross(F, Ev, c, cs);
      CrossCfg v = c;
      v.partials = false; v.check = false; v.cnt = true; v.launches = 2;
      const CrossRes r = run_cross(F, Ev, v, cs + " in-kernel combine x2");
      F.result(cs + " in-kernel combine == separate", r.out == base.out, r.out == base.out ? 0 : INFINITY);
      for (int cn = 0; cn < 2; ++cn) {
        CrossCfg w = c;
        w.partials = false; w.done = 2; w.cnt = cn; w.launches = cn ? 2 : 1;
        run_cross(F, Ev, w, cs + " done+group" + (cn ? " cnt" : ""));
      }
    }
  {
    CrossCfg c;                // 33 rows per window is past the matrix-core decode form: the group kernel takes it
    c.rows = 33; c.group = 33; c.mfma = 1; c.gen_shift = k++;
    run_cross(F, E, c, "decode group 33 (falls to the group kernel)");
  }
  return F.finish();
}

// ==================================================================================================================
// The factored form (attn_xenc.hip): one environment per n_state
struct XEnv {
  int d = 0, H = 0, T = T_ENC, NS = 0, qw = 0, nw = 0;
  std::vector<uint16_t> E;               // [slot][T][d] row-major
  std::vector<double> Ed, E8d;           // f64 of the bf16 values / of the decoded e4m3 x scale values
  DBuf dErm, dEblk, dE8, dEscale;
  // grid = the key-split count whose split edges carry the EDGES spikes (tiles [s 47 / grid, (s + 1) 47 / grid))
  void make(Fam& F, int d_, int NS_, uint64_t seed, int grid = 16) {
    d = d_; H = d / HD; NS = NS_;
    xgeometry(d, qw, nw);
    int dq = 0, dn = 0;
    xattn_geometry(d, dq, dn);
    F.result("geometry d " + std::to_string(d), dq == qw && dn == nw, dq == qw && dn == nw ? 0 : INFINITY);
    std::vector<int> bounds;
    for (int s2 = 0; s2 < grid; ++s2) bounds.push_back(s2 * 47 / grid * 32);
    E.resize((size_t)NS * T * d);
    Rng g(seed);
    std::vector<uint16_t> k(d), v(d);
    for (int sl = 0; sl < NS; ++sl)
      for (int t = 0; t < T; ++t) {
        gen_key_row(g, t, T, THR_X, bounds, 8, k.data());
        gen_val_row(g, d, false, v.data());
        uint16_t* row = &E[((size_t)sl * T + t) * d];
        for (int c = 0; c < d; ++c) row[c] = c < 8 ? k[c] : v[c];
        if (sl == NS - 1 && t == 700) std::fill(row, row + d, (uint16_t)0);     // an all-zero position (fp8 scale 0)
      }
    Ed.resize(E.size());
    for (size_t i = 0; i < E.size(); ++i) Ed[i] = b2f(E[i]);
    dErm.put(E);
    // blocked slots from launch_xblock, checked against the index formula (rows past T are zeros)
    const long long se = xslot_elems(T, d);
    F.result("xblock_slot_elems d " + std::to_string(d), xblock_slot_elems(T, d) == se, xblock_slot_elems(T, d) == se ? 0 : INFINITY);
    dEblk.sentinel_fill((size_t)NS * se * 2);
    launch("launch_xblock", [&] { launch_xblock(dErm.p<bf16>(), NS, T, d, dEblk.p<bf16>(), true, nullptr); });
    {
      std::vector<uint16_t> want((size_t)NS * se, 0);
      for (int sl = 0; sl < NS; ++sl)
        for (int t = 0; t < T; ++t)
          for (int c = 0; c < d; ++c) want[(size_t)sl * se + xblocked_index(t, c, d)] = E[((size_t)sl * T + t) * d + c];
      const auto got = dEblk.get();
      const bool same = std::memcmp(got.data(), want.data(), got.size()) == 0;
      F.result("xblock layout d " + std::to_string(d), same, same ? 0 : INFINITY);
      DBuf back;
      back.sentinel_fill((size_t)NS * T * d * 2);
      launch("launch_xblock", [&] { launch_xblock(dEblk.p<bf16>(), NS, T, d, back.p<bf16>(), false, nullptr); });
      const auto rt = back.get();
      const bool same2 = std::memcmp(rt.data(), E.data(), rt.size()) == 0;
      F.result("xblock round trip d " + std::to_string(d), same2, same2 ? 0 : INFINITY);
      F.guards("xblock d " + std::to_string(d), {&dErm, &dEblk, &back});
    }
  }
  void make_f8(Fam& F) {
    dE8.sentinel_fill((size_t)NS * T * d);
    dEscale.sentinel_fill((size_t)NS * T * 4);
    launch("launch_xquant8", [&] { launch_xquant8(dErm.p<bf16>(), (long long)NS * T, d, dE8.p<unsigned char>(), dEscale.p<float>(), nullptr); });
    const auto codes = dE8.get(), sb = dEscale.get();
    E8d.resize(E.size());
    double worst = 0;
    for (size_t r = 0; r < (size_t)NS * T; ++r) {
      float sc;
      std::memcpy(&sc, &sb[r * 4], 4);
      for (int c = 0; c < d; ++c) {
        const double v = e4m3(codes[r * d + c]) * (double)sc;
        E8d[r * d + c] = v;
        // the quantiser itself: within half an e4m3 step (2^-4 relative, 2^-10 x 448 of the row maximum below the normals)
        worst = std::max(worst, std::fabs(v - Ed[r * d + c]) / (std::ldexp(std::fabs(Ed[r * d + c]), -4) + std::ldexp((double)sc, -10) + 1e-6 * std::fabs(Ed[r * d + c]) + 1e-300));
      }
    }
    F.result("xquant8 d " + std::to_string(d), worst <= 1.0, worst);
    F.guards("xquant8", {&dE8, &dEscale});
  }
};

struct XCfg {
  int rows = 1, group = 1, splits = 1, done = 0, gen = -1 /* mixed */, gen_shift = 0, rev = 0, keep = 0;
  bool f8 = false, cap = false, check = true;
};
struct XRes {
  std::vector<uint8_t> pu, pml, probs;
};
static XRes run_xattn(Fam& F, XEnv& X, const XCfg& c, const std::string& cs) {
  const int d = X.d, H = X.H, T = X.T, rows = c.rows, group = c.group, S = c.splits;
  const long long slab_rows = rows + 3;
  const int n_align = 4;
  std::vector<int> head_map(H, -1), row_hyp(rows), hyp_slot(rows), done(rows, 0);
  head_map[0] = 1; head_map[H - 1] = 0; if (H > 3) head_map[3] = 2;
  for (int r = 0; r < rows; ++r) row_hyp[r] = rows - 1 - r;
  for (int hy = 0; hy < rows; ++hy) {
    hyp_slot[hy] = ((rows - 1 - hy) / group) % X.NS;           // several groups share a slot when there are more than NS
    if (c.done) done[hy] = hy % 3 == 1;
  }
  if (c.done >= 2)
    for (int r = 0; r < group; ++r) done[row_hyp[r]] = 1;
  std::vector<uint16_t> qp((size_t)rows * H * d);
  {
    Rng g(5000 + d + rows * 7 + c.gen_shift);
    for (int r = 0; r < rows; ++r)
      for (int h = 0; h < H; ++h)
        gen_query(g, c.gen >= 0 ? c.gen : mixed_gen(r * H + h + c.gen_shift), d, 1.0 / LN2, &qp[((size_t)r * H + h) * d], 1.0 / std::sqrt((double)d));
  }
  DBuf dqp, drh, dhs, ddone, dhm, dpu, dpml, dprobs;
  dqp.put(qp); drh.put(row_hyp); dhs.put(hyp_slot); ddone.put(done); dhm.put(head_map);
  const size_t n_u = (size_t)S * H * d * slab_rows, n_ml = (size_t)S * slab_rows * H * 2;
  dpu.sentinel_fill(n_u * 2); dpml.sentinel_fill(n_ml * 4);
  if (c.cap) dprobs.sentinel_fill((size_t)(rows + 1) * n_align * T * 4);
  launch("launch_xattn", [&] {
    launch_xattn(dqp.p<bf16>(), c.f8 ? (const void*)X.dE8.p<unsigned char>() : (const void*)X.dEblk.p<bf16>(),
                 c.f8 ? X.dEscale.p<float>() : nullptr, dhs.p<int>(), drh.p<int>(), c.done ? ddone.p<int>() : nullptr, rows, slab_rows, group,
                 H, T, d, S, c.rev, c.keep, dpu.p<bf16>(), dpml.p<float>(), c.cap ? dprobs.p<float>() : nullptr,
                 c.cap ? dhm.p<int>() : nullptr, n_align, nullptr, nullptr, nullptr, nullptr);
  });
  XRes res;
  res.pu = dpu.get(); res.pml = dpml.get();
  if (c.cap) res.probs = dprobs.get();
  F.guards(cs, {&dqp, &drh, &dhs, &ddone, &dhm, &dpu, &dpml, &dprobs, &X.dEblk, &X.dE8, &X.dEscale});
  if (!c.check) return res;

  Timer tm;
  const std::vector<double>& Ed = c.f8 ? X.E8d : X.Ed;
  const int n_tiles = (T + 31) / 32;
  std::vector<long long> all(T);
  for (int t = 0; t < T; ++t) all[t] = t;
  Image iu(n_u), iml(n_ml), ip(c.cap ? (size_t)(rows + 1) * n_align * T : 0);
  std::vector<Worst> wl(rows * H), wp(rows * H);
  parallel_for(rows * H, [&](int i) {
    const int r = i / H, h = i % H;
    if (c.done && done[row_hyp[r]]) return;
    const int slot = hyp_slot[row_hyp[r - r % group]];
    std::vector<double> q(d);
    for (int x = 0; x < d; ++x) q[x] = b2f(qp[((size_t)r * H + h) * d + x]);
    const double* Es = &Ed[(size_t)slot * T * d];
    for (int s = 0; s < S; ++s) {
      const int b = s * n_tiles / S * 32, e = std::min(T, (s + 1) * n_tiles / S * 32);
      Att a;
      attend(q.data(), d, 1.0, Es, d, Es, d, d, all.data() + b, e - b, d + X.nw + (c.f8 ? 1 : 0), a);
      for (int x = 0; x < d; ++x) {
        const size_t ix = (size_t)part_u_index(s, r, h, x, H, d, slab_rows);
        iu.ref[ix] = a.o[x];
        iu.tol[ix] = tol_out(a.o[x], a.A[x], a.ds, a.n, true, a.vmax[x]);
      }
      const size_t im = (size_t)part_ml_index(s, r, h, H, slab_rows);
      iml.tol[im] = iml.tol[im + 1] = INFINITY;            // written; checked through the LSE form below
      float m, l;
      std::memcpy(&m, &res.pml[im * 4], 4);
      std::memcpy(&l, &res.pml[im * 4 + 4], 4);
      wl[i].see(std::fabs((double)m + std::log2((double)l) - a.lse), tol_lse(a.lse, a.ds, a.n), (long long)im);
      const double slack = 2 * a.ds + 2 * U24 * std::fabs(a.smax);
      if (!(m <= a.smax + slack && m >= a.smax - THR_X - slack)) wl[i].see(INFINITY, 1, (long long)im);
      if (c.cap && head_map[h] >= 0)
        for (int t = b; t < e; ++t) {
          const size_t ix = ((size_t)r * n_align + head_map[h]) * T + t;
          ip.ref[ix] = a.s[t - b];
          ip.tol[ix] = 2.0 * ((d + X.nw + 2) * U24 * a.sabs[t - b] + U24 * std::fabs(a.s[t - b]));
        }
    }
  });
  const Cmp cu = compare<uint16_t>(iu, res.pu);
  F.result(cs + " u/l", cu.ok(), cu.w.ratio, cu.str());
  const Cmp cm = compare<float>(iml, res.pml);
  Worst w;
  for (auto& x : wl) if (x.at >= 0) w.merge(x);
  F.result(cs + " (m, l) LSE form", w.ok() && cm.sentinel_bad == 0, w.ratio, cm.sentinel_bad ? cm.str() : "worst at record " + std::to_string(w.at));
  if (c.cap) {
    const Cmp cp = compare<float>(ip, res.probs);
    F.result(cs + " captured scores", cp.ok(), cp.w.ratio, cp.str());
  }
  return res;
}

static int fam_xattn() {
  Fam F{"xattn"};
  int k = 0;
  {
    XEnv X;
    X.make(F, 384, 3, 31);
    X.make_f8(F);
    struct Occ { int rows, group; };
    // G H = 6 (6 valid lanes of 32), 5 groups over 3 slots; G H = 96: three full m-tiles, two groups
    for (const Occ oc : {Occ{5, 1}, Occ{32, 16}}) {
      XRes base3;
      for (int S : {1, 2, 3, 5, 8, 16})
        for (int dn : {0, 2}) {
          XCfg c;
          c.rows = oc.rows; c.group = oc.group; c.splits = S; c.done = dn; c.gen_shift = k;
          const std::string cs = "d 384 rows " + std::to_string(oc.rows) + " group " + std::to_string(oc.group) + " splits " + std::to_string(S) + (dn ? " done" : "");
          const XRes r = run_xattn(F, X, c, cs);
          if (S == 3 && dn == 2) {
            for (int v = 1; v < 4; ++v) {          // the item order (rev) and the load policy (keep) change no bit
              XCfg cv = c;
              cv.rev = v & 1; cv.keep = v >> 1; cv.check = false;
              const XRes rv = run_xattn(F, X, cv, cs + " rev/keep");
              const bool same = rv.pu == r.pu && rv.pml == r.pml;
              F.result(cs + " rev " + std::to_string(v & 1) + " keep " + std::to_string(v >> 1) + " == base", same, same ? 0 : INFINITY);
            }
          }
        }
      ++k;
      // every generator alone in a tile (a uniform vote), then capture, then the fp8 cross memory
      for (int gen = 0; gen < N_GEN; ++gen) {
        XCfg c;
        c.rows = oc.rows; c.group = oc.group; c.splits = 3; c.gen = gen;
        run_xattn(F, X, c, "d 384 rows " + std::to_string(oc.rows) + " " + gen_name(gen) + " splits 3");
      }
      for (int S : {1, 5}) {
        XCfg c;
        c.rows = oc.rows; c.group = oc.group; c.splits = S; c.cap = true; c.done = 1; c.gen_shift = k++;
        run_xattn(F, X, c, "d 384 rows " + std::to_string(oc.rows) + " capture splits " + std::to_string(S));
      }
      for (int gen : {(int)PLAIN, (int)STAIRS, -1}) {
        XCfg c;
        c.rows = oc.rows; c.group = oc.group; c.splits = 3; c.gen = gen; c.f8 = true; c.gen_shift = k++;
        run_xattn(F, X, c, "d 384 rows " + std::to_string(oc.rows) + " fp8 " + (gen < 0 ? "mixed" : gen_name(gen)));
      }
    }
    // every generator alone at every split count, on an E whose EDGES spikes sit on THAT count's split edges (maxima
    // of neighbouring splits 159 log2 units apart in the partials themselves)
    for (int S : {2, 3, 5, 8, 16}) {
      XEnv XS;
      XS.make(F, 384, 2, 33 + S, S);
      for (int gen = 0; gen < N_GEN; ++gen) {
        XCfg c;
        c.rows = 10; c.group = 5; c.splits = S; c.gen = gen; c.gen_shift = k++;
        run_xattn(F, XS, c, std::string("d 384 rows 10 group 5 ") + gen_name(gen) + " splits " + std::to_string(S) + " (edges on this grid)");
      }
    }
    DBuf z;
    z.zero_fill(1 << 16);
    const bool t1 = throws([&] {
      launch_xattn(z.p<bf16>(), X.dEblk.p<bf16>(), nullptr, z.p<int>(), z.p<int>(), nullptr, 1, 1, 1, 6, T_ENC, 384, 48, 0, 0, z.p<bf16>(),
                   z.p<float>(), nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    });
    F.result("splits 48 refused", t1, t1 ? 0 : INFINITY);
    const bool t2 = throws([&] {
      launch_xattn(z.p<bf16>(), X.dEblk.p<bf16>(), nullptr, z.p<int>(), z.p<int>(), nullptr, 7, 7, 5, 6, T_ENC, 384, 1, 0, 0, z.p<bf16>(),
                   z.p<float>(), nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    });
    F.result("rows % group != 0 refused", t2, t2 ? 0 : INFINITY);
  }
  for (int d : {512, 768, 1024, 1280}) {
    XEnv X;
    X.make(F, d, 2, 40 + d);
    const int G = d == 1280 ? 5 : 2;          // d = 1280: G H = 100, a fourth m-tile with 4 valid lanes
    for (int S : {1, 3})
      for (int gen : {(int)STAIRS, -1}) {
        XCfg c;
        c.rows = 2 * G; c.group = G; c.splits = S; c.gen = gen; c.done = gen < 0 ? 1 : 0; c.gen_shift = k++;
        run_xattn(F, X, c, "d " + std::to_string(d) + " rows " + std::to_string(2 * G) + " splits " + std::to_string(S) + (gen < 0 ? " mixed" : " stairs"));
      }
  }
  return F.finish();
}

// ==================================================================================================================
// Random projection weights of one layer and their packed forms (launch_xpack, checked against the index formulas)
struct XW {
  int d = 0, H = 0;
  std::vector<uint16_t> ckv;             // [K | V][d][d]
  std::vector<float> bv;
  DBuf dckv, dwkt, dwvb, dbv;
  // selectors: Wk row h 64 + j is the unit vector of column j for j < 8 (and no other row reaches columns 0..7), so
  // element j of a head's q drives profile channel j of E exactly as in the head form (q' = q / 8 log2 e)
  void make(Fam& F, int d_, uint64_t seed, double wscale, bool selectors = false) {
    d = d_; H = d / HD;
    ckv.resize((size_t)2 * d * d);
    bv.resize(d);
    Rng g(seed);
    for (auto& x : ckv) x = f2b((float)(g.randn() * wscale));
    if (selectors)
      for (int r = 0; r < d; ++r)
        for (int c = 0; c < d; ++c)
          if (c < 8 || r % HD < 8) ckv[(size_t)r * d + c] = f2b(r % HD == c ? 1.0f : 0.0f);
    for (auto& x : bv) x = (float)(g.randn() * 0.1);
    dckv.put(ckv); dbv.put(bv);
    dwkt.sentinel_fill((size_t)d * d * 2); dwvb.sentinel_fill((size_t)d * d * 2);
    launch("launch_xpack", [&] { launch_xpack(dckv.p<bf16>(), dwkt.p<bf16>(), dwvb.p<bf16>(), 1, H, d, nullptr); });
    std::vector<uint16_t> wk((size_t)d * d), wv((size_t)d * d);
    for (int h = 0; h < H; ++h)
      for (int j = 0; j < HD; ++j)
        for (int c = 0; c < d; ++c) {
          wk[(size_t)wkt_index(h, j, c, d)] = ckv[((size_t)h * HD + j) * d + c];
          wv[(size_t)wvb_index(h, j, c, d)] = ckv[((size_t)d + h * HD + j) * d + c];
        }
    const auto gk = dwkt.get(), gv = dwvb.get();
    const bool same = std::memcmp(gk.data(), wk.data(), gk.size()) == 0 && std::memcmp(gv.data(), wv.data(), gv.size()) == 0;
    F.result("xpack layouts d " + std::to_string(d), same, same ? 0 : INFINITY);
    F.guards("xpack", {&dckv, &dwkt, &dwvb});
  }
  double wk(int row, int c) const { return b2f(ckv[(size_t)row * d + c]); }
  double wv(int row, int c) const { return b2f(ckv[((size_t)d + row) * d + c]); }
};

static int fam_xq() {
  Fam F{"xq"};
  int k = 0;
  for (int d : {384, 512, 768, 1024, 1280}) {
    XW W;
    W.make(F, d, 60 + d, 0.05);
    const int H = W.H;
    for (int rows : {1, 31, 32, 33, 70}) {
      const long long ldq = d + 8;
      std::vector<uint16_t> q((size_t)rows * ldq);
      Rng g(7000 + d + rows);
      for (auto& x : q) x = f2b((float)(g.randn() * NOISE));
      // reference: q'[r][h][c] = scale sum_j Wk[h 64 + j][c] q[r][h 64 + j]; 64 accumulations + the scale
      auto check = [&](const std::vector<uint16_t>& qh, const std::vector<uint8_t>& got, const std::string& cs) {
        Timer tm;
        Image im((size_t)(rows + 1) * H * d);
        parallel_for(rows, [&](int r) {
          for (int h = 0; h < H; ++h)
            for (int c = 0; c < d; ++c) {
              double a = 0, b = 0;
              for (int j = 0; j < HD; ++j) {
                const double x = W.wk(h * HD + j, c) * b2f(qh[(size_t)r * ldq + h * HD + j]);
                a += x; b += std::fabs(x);
              }
              const size_t i = ((size_t)r * H + h) * d + c;
              im.ref[i] = a * scale_log2();
              im.tol[i] = 2 * U9 * std::fabs(im.ref[i]) + 2.0 * (HD + 1) * U24 * b * scale_log2();
            }
        });
        const Cmp cmp = compare<uint16_t>(im, got);
        F.result(cs, cmp.ok(), cmp.w.ratio, cmp.str());
      };
      DBuf dq, dqp, dslab, dbias;
      auto run = [&](const std::vector<uint16_t>& qh, const CrossFuse& fz) {
        dq.put(qh);
        dqp.sentinel_fill((size_t)(rows + 1) * H * d * 2);
        launch("launch_xq", [&] { launch_xq(fz.q_part ? nullptr : dq.p<bf16>(), ldq, fz, W.dwkt.p<bf16>(), dqp.p<bf16>(), rows, H, d, nullptr); });
        auto got = dqp.get();
        F.guards("xq", {&dq, &dqp, &dslab, &dbias, &W.dwkt});
        return got;
      };
      const std::string cs = "d " + std::to_string(d) + " rows " + std::to_string(rows);
      check(q, run(q, CrossFuse{}), cs);
      static const int SL[3] = {1, 4, 16};
      for (int sl : rows == 33 ? std::vector<int>{1, 4, 16} : std::vector<int>{SL[k++ % 3]}) {
        const int q_rows = rows + 2;
        std::vector<float> slab((size_t)sl * q_rows * ldq), bias(d);
        for (auto& x : slab) x = (float)(g.randn() * NOISE / std::sqrt((double)sl));
        for (auto& x : bias) x = (float)(g.randn() * 0.1);
        std::vector<uint16_t> qs((size_t)rows * ldq, 0);
        for (int r = 0; r < rows; ++r)
          for (int i = 0; i < d; ++i) {
            float v = 0.f;
            for (int s2 = 0; s2 < sl; ++s2) v += slab[((size_t)s2 * q_rows + r) * ldq + i];
            qs[(size_t)r * ldq + i] = f2b(v + bias[i]);
          }
        dslab.put(slab); dbias.put(bias);
        CrossFuse fz;
        fz.q_part = dslab.p<float>(); fz.q_splits = sl; fz.q_rows = q_rows; fz.q_bias = dbias.p<float>();
        const auto fused = run(qs, fz);
        const auto plain = run(qs, CrossFuse{});
        check(qs, plain, cs + " host-summed q of " + std::to_string(sl) + " slabs");
        F.result(cs + " slabs " + std::to_string(sl) + " fused == plain", fused == plain, fused == plain ? 0 : INFINITY);
      }
    }
  }
  {
    DBuf z;
    z.zero_fill(1 << 16);
    const bool th = throws([&] { launch_xq(z.p<bf16>(), 640, CrossFuse{}, z.p<bf16>(), z.p<bf16>(), 1, 10, 640, nullptr); });
    F.result("d = 640 refused", th, th ? 0 : INFINITY);
  }
  return F.finish();
}

// ==================================================================================================================
// xcomb: launch_xcomb_vo alone on synthesised partials
static int fam_xcomb() {
  Fam F{"xcomb"};
  const int T = T_ENC, n_align = 4;
  int k = 0;
  for (int d : {384, 512, 768, 1024, 1280}) {
    XW W;
    W.make(F, d, 80 + d, 0.05);
    const int H = W.H;
    std::vector<int> head_map(H, -1);
    head_map[1] = 0; head_map[H - 1] = 2;
    DBuf dhm;
    dhm.put(head_map);
    auto one = [&](int rows, int S, int spread, bool wd, bool cap, std::vector<uint8_t>* keep_out, const std::vector<uint8_t>* first40) {
      const long long slab_rows = rows + 2;
      const size_t n_u = (size_t)S * H * d * slab_rows, n_ml = (size_t)S * slab_rows * H * 2;
      std::vector<uint16_t> pu(n_u);
      std::vector<float> pml(n_ml);
      // (seeded by the shape only up to the first 40 rows' values: a record's value depends on (s, row, h, c) alone)
      auto hash = [](uint64_t a) { Rng r(a); return r; };
      for (int s = 0; s < S; ++s)
        for (int r = 0; r < slab_rows; ++r)
          for (int h = 0; h < H; ++h) {
            Rng g = hash(((uint64_t)d * 131 + s) * 1000003 + (uint64_t)r * 257 + h + 17 * spread);
            const double base = -40.0 + 3.0 * (r % 7);
            const double m = spread == 0 ? base : spread == 1 ? base - 7.0 * g.uni() : base - (s % 2 ? 160.0 + 5 * g.uni() : g.uni());
            const size_t im = (size_t)part_ml_index(s, r, h, H, slab_rows);
            pml[im] = (float)m;
            pml[im + 1] = (float)(1.0 + 49.0 * g.uni());
            for (int c = 0; c < d; ++c) pu[(size_t)part_u_index(s, r, h, c, H, d, slab_rows)] = f2b((float)(g.randn() * 0.4));
          }
      std::vector<int> row_hyp(rows), done(rows, 0);
      for (int r = 0; r < rows; ++r) row_hyp[r] = rows - 1 - r;
      if (wd) for (int hy = 0; hy < rows; ++hy) done[hy] = hy % 3 == 1;
      std::vector<float> probs;
      if (cap) {
        probs.resize((size_t)(rows + 1) * n_align * T);
        Rng g(900 + rows + S);
        for (auto& x : probs) x = (float)(-45.0 - 30.0 * g.uni());
      }
      DBuf dpu, dpml, drh, ddone, dout, dprobs;
      dpu.put(pu); dpml.put(pml); drh.put(row_hyp); ddone.put(done);
      const long long ldo = d;
      dout.sentinel_fill((size_t)(rows + 1) * ldo * 2);
      std::vector<uint8_t> probs_in;
      if (cap) {
        // unmapped slots, finished rows and the row past the end keep the sentinel; mapped live rows hold raw scores
        dprobs.sentinel_fill(probs.size() * 4);
        probs_in = dprobs.get();
        for (int r = 0; r < rows; ++r)
          for (int h = 0; h < H; ++h)
            if (head_map[h] >= 0 && !(wd && done[row_hyp[r]]))
              std::memcpy(&probs_in[(((size_t)r * n_align + head_map[h]) * T) * 4], &probs[((size_t)r * n_align + head_map[h]) * T], (size_t)T * 4);
        CK(hipMemcpy(dprobs.p<uint8_t>(), probs_in.data(), probs_in.size(), hipMemcpyHostToDevice));
      }
      launch("launch_xcomb_vo", [&] {
        launch_xcomb_vo(dpu.p<bf16>(), dpml.p<float>(), S, slab_rows, W.dwvb.p<bf16>(), W.dbv.p<float>(), drh.p<int>(), wd ? ddone.p<int>() : nullptr,
                        dout.p<bf16>(), ldo, rows, H, d, T, cap ? dprobs.p<float>() : nullptr, cap ? dhm.p<int>() : nullptr, n_align, nullptr);
      });
      const auto got = dout.get();
      const std::string cs = "d " + std::to_string(d) + " rows " + std::to_string(rows) + " splits " + std::to_string(S) + " spread " +
                             (spread == 0 ? "0" : spread == 1 ? "7" : ">150") + (wd ? " done" : "") + (cap ? " capture" : "");
      F.guards(cs, {&dpu, &dpml, &drh, &ddone, &dout, &dprobs, &W.dwvb, &W.dbv});
      if (keep_out) *keep_out = got;
      if (first40) {       // the 32-row block form gives the 16-row form's bits
        const bool same = std::memcmp(got.data(), first40->data(), (size_t)40 * ldo * 2) == 0;
        F.result(cs + " first 40 rows == the rows 40 launch", same, same ? 0 : INFINITY);
        return;
      }
      Timer tm;
      Image im((size_t)(rows + 1) * ldo), ip(cap ? probs.size() : 0);
      parallel_for(rows, [&](int r) {
        if (wd && done[row_hyp[r]]) return;
        for (int h = 0; h < H; ++h) {
          double M = -INFINITY, L = 0, w[16];
          for (int s = 0; s < S; ++s) M = std::max(M, (double)pml[(size_t)part_ml_index(s, r, h, H, slab_rows)]);
          for (int s = 0; s < S; ++s) {
            const size_t i2 = (size_t)part_ml_index(s, r, h, H, slab_rows);
            w[s] = (double)pml[i2 + 1] * std::exp2((double)pml[i2] - M);
            L += w[s];
          }
          std::vector<double> u(d, 0.0), ua(d, 0.0);
          for (int s = 0; s < S; ++s)
            for (int c = 0; c < d; ++c) {
              const double x = w[s] / L * b2f(pu[(size_t)part_u_index(s, r, h, c, H, d, slab_rows)]);
              u[c] += x; ua[c] += std::fabs(x);
            }
          // rounding steps: the weight (exp2 2 ulp, x l, x 1/L, the sum L: S + 4), the merge's S fmas, d MFMA accumulations,
          // the 8-wave sum and the bias (9); the bf16 hi + lo split of the merged u leaves 2^-8 x 2^-8 of it (u^2, negligible)
          const double kap = 2.0 * ((2 * S + 4 + d + 9) * U24 + std::ldexp(1.0, -16));
          for (int j = 0; j < HD; ++j) {
            double o = 0, B = 0;
            for (int c = 0; c < d; ++c) { o += u[c] * W.wv(h * HD + j, c); B += ua[c] * std::fabs(W.wv(h * HD + j, c)); }
            const size_t i2 = (size_t)r * ldo + h * HD + j;
            im.ref[i2] = o + W.bv[h * HD + j];
            im.tol[i2] = 2 * U9 * std::fabs(im.ref[i2]) + kap * (B + std::fabs((double)W.bv[h * HD + j]));
          }
          if (cap && head_map[h] >= 0)
            for (int t = 0; t < T; ++t) {
              const size_t i2 = ((size_t)r * n_align + head_map[h]) * T + t;
              // the kernel's own merged (M, L) in f32: exp2 (2 ulp), the subtraction, the division, L's S + 2 steps
              ip.ref[i2] = std::exp2((double)probs[i2] - M) / L;
              ip.tol[i2] = 2.0 * ip.ref[i2] * ((S + 8) * U24 + LN2 * U24 * std::fabs((double)probs[i2] - M)) + std::ldexp(1.0, -126);
            }
        }
      });
      const Cmp c1 = compare<uint16_t>(im, got);
      F.result(cs, c1.ok(), c1.w.ratio, c1.str());
      if (cap) {
        const Cmp c2 = compare<float>(ip, dprobs.get());
        F.result(cs + " probs", c2.ok(), c2.w.ratio, c2.str());
      }
    };
    for (int rows : {1, 15, 16, 17, 40})
      for (int S : {1, 2, 3, 4, 5, 8, 9, 16}) {
        const int spread = k++ % 3;
        one(rows, S, spread, rows >= 15 && (k & 1), false, nullptr, nullptr);
      }
    for (int S : {1, 3, 9}) one(17, S, 2, true, true, nullptr, nullptr);
    if (d == 1280) {
      std::vector<uint8_t> r40;
      one(40, 3, 2, false, false, &r40, nullptr);
      one(400, 3, 2, false, false, nullptr, &r40);
    }
  }
  return F.finish();
}

// ==================================================================================================================
// xchain: xq -> xattn -> xcomb_vo with the split count of xattn_splits, against the PROJECTED definition
// (K = E Wk^T, V = E Wv^T + bv) in f64.  The device rounds q' to bf16 (and forms it in f32) before the attention; the
// reference keeps it exact, so the bound adds that perturbation.  |dq'_c| <= 2 U9 |q'_c| + 2 (64 + 1) U24 qabs_c (the
// bf16 store and xq's f32 sum, both doubled) moves score t by at most sum_c |dq'_c| |E_tc|; a softmax only sees score
// DIFFERENCES, so against the row's top key t* the shift is D_t = sum_c |dq'_c| |E_tc - E_t*c| and, with
// g = sum_t p_t (2^D_t - 1) and G_c = sum_t p_t (2^D_t - 1) |E_tc|,  |u'_c - u_c| <= (G_c + |u_c| g) / (1 - g)   (rigorous
// for g < 1: numerator and denominator of the perturbed softmax bounded separately).  A case where this term alone
// exceeds 2^-4 of the row's largest |ref| says nothing: it is printed as "loose" and fails the family.
static int fam_xchain() {
  Fam F{"xchain"};
  const int T = T_ENC;
  int k = 0;
  for (int d : {384, 1280}) {
    XEnv X;
    X.make(F, d, 2, 90 + d);
    XW W;
    W.make(F, d, 95 + d, 0.05, true);
    const int H = X.H;
    for (int group : {1, 5})
      for (int gen : {(int)STAIRS, -1}) {
        const int rows = group == 1 ? 3 : 10;
        const std::string cs = "d " + std::to_string(d) + " rows " + std::to_string(rows) + " group " + std::to_string(group) + (gen < 0 ? " mixed" : " stairs");
        std::vector<uint16_t> q((size_t)rows * d);
        // (a small q noise: the q' rounding term sums |dq'_c| |E_tc - E_t*c| over all d columns without cancellation, and
        // on the flat and plain rows of a mixed tile it would otherwise pass 2^-4 of the output: chosen on the CPU)
        Rng g(9000 + d + group + k++);
        for (int r = 0; r < rows; ++r)
          for (int h = 0; h < H; ++h) gen_query(g, gen >= 0 ? gen : mixed_gen(r * H + h), HD, 8.0, &q[(size_t)r * d + h * HD], NOISE / 32);
        std::vector<int> row_hyp(rows), hyp_slot(rows);
        for (int r = 0; r < rows; ++r) { row_hyp[r] = rows - 1 - r; hyp_slot[r] = ((rows - 1 - r) / group) % X.NS; }
        const int S = xattn_splits(rows, group, H, T, d);
        DBuf dq, dqp, drh, dhs, dpu, dpml, dout;
        dq.put(q); drh.put(row_hyp); dhs.put(hyp_slot);
        dqp.sentinel_fill((size_t)rows * H * d * 2);
        const long long slab_rows = rows + 2;
        dpu.sentinel_fill((size_t)S * H * d * slab_rows * 2);
        dpml.sentinel_fill((size_t)S * slab_rows * H * 2 * 4);
        dout.sentinel_fill((size_t)(rows + 1) * d * 2);
        launch("launch_xq", [&] { launch_xq(dq.p<bf16>(), d, CrossFuse{}, W.dwkt.p<bf16>(), dqp.p<bf16>(), rows, H, d, nullptr); });
        launch("launch_xattn", [&] {
          launch_xattn(dqp.p<bf16>(), X.dEblk.p<bf16>(), nullptr, dhs.p<int>(), drh.p<int>(), nullptr, rows, slab_rows, group, H, T, d, S, 0, 0,
                       dpu.p<bf16>(), dpml.p<float>(), nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
        });
        launch("launch_xcomb_vo", [&] {
          launch_xcomb_vo(dpu.p<bf16>(), dpml.p<float>(), S, slab_rows, W.dwvb.p<bf16>(), W.dbv.p<float>(), drh.p<int>(), nullptr, dout.p<bf16>(), d,
                          rows, H, d, T, nullptr, nullptr, 0, nullptr);
        });
        const auto got = dout.get();
        F.guards(cs, {&dq, &dqp, &drh, &dhs, &dpu, &dpml, &dout, &X.dEblk, &W.dwkt, &W.dwvb, &W.dbv});
        {
          // the partial slabs between the two kernels: records of rows >= rows keep their sentinel
          Image iu((size_t)S * H * d * slab_rows), iml((size_t)S * slab_rows * H * 2);
          for (int s2 = 0; s2 < S; ++s2)
            for (int r = 0; r < rows; ++r)
              for (int h = 0; h < H; ++h) {
                for (int c = 0; c < d; ++c) iu.tol[(size_t)part_u_index(s2, r, h, c, H, d, slab_rows)] = INFINITY;
                const size_t im2 = (size_t)part_ml_index(s2, r, h, H, slab_rows);
                iml.tol[im2] = iml.tol[im2 + 1] = INFINITY;
              }
          const size_t bad = compare<uint16_t>(iu, dpu.get()).sentinel_bad + compare<float>(iml, dpml.get()).sentinel_bad;
          F.result(cs + " partial slabs outside the write set", bad == 0, bad ? INFINITY : 0, std::to_string(bad) + " bytes changed");
        }
        Timer tm;
        Image im((size_t)(rows + 1) * d);
        std::vector<double> pert_row(rows, 0.0), refmax_row(rows, 0.0);
        std::vector<std::vector<double>> pert((size_t)rows * H, std::vector<double>(HD, 0.0));
        std::vector<long long> all(T);
        for (int t = 0; t < T; ++t) all[t] = t;
        parallel_for(rows * H, [&](int i) {
          const int r = i / H, h = i % H;
          const double* Es = &X.Ed[(size_t)hyp_slot[row_hyp[r - r % group]] * T * d];
          std::vector<double> qx(d), dqx(d);
          for (int c = 0; c < d; ++c) {
            double a = 0, b = 0;
            for (int j = 0; j < HD; ++j) {
              const double x = W.wk(h * HD + j, c) * b2f(q[(size_t)r * d + h * HD + j]);
              a += x; b += std::fabs(x);
            }
            qx[c] = a * scale_log2();
            dqx[c] = 2 * U9 * std::fabs(qx[c]) + 2.0 * (HD + 1) * U24 * b * scale_log2();
          }
          Att a;
          attend(qx.data(), d, 1.0, Es, d, Es, d, d, all.data(), T, d + X.nw, a);
          int ts = 0;
          for (int t = 1; t < T; ++t) if (a.s[t] > a.s[ts]) ts = t;
          double gsum = 0;
          std::vector<double> G(d, 0.0);
          for (int t = 0; t < T; ++t) {
            if (a.p[t] == 0.0) continue;
            double D = 0;
            for (int c = 0; c < d; ++c) D += dqx[c] * std::fabs(Es[(size_t)t * d + c] - Es[(size_t)ts * d + c]);
            const double f = a.p[t] * (std::exp2(D) - 1.0);
            gsum += f;
            for (int c = 0; c < d; ++c) G[c] += f * std::fabs(Es[(size_t)t * d + c]);
          }
          std::vector<double> tu(d), pu(d);
          for (int c = 0; c < d; ++c) {
            pu[c] = gsum < 1.0 ? (G[c] + std::fabs(a.o[c]) * gsum) / (1.0 - gsum) : INFINITY;
            // the attention's own bound on u (P in bf16) + the bf16 store of each split's u / l
            tu[c] = tol_out(0.0, a.A[c], a.ds, a.n, true, a.vmax[c]) + 2 * U9 * a.A[c];
          }
          const double kap = 2.0 * ((2 * S + 4 + d + 9) * U24 + std::ldexp(1.0, -16));      // as xcomb
          for (int j = 0; j < HD; ++j) {
            double o = 0, B = 0, tj = 0, pj = 0;
            for (int c = 0; c < d; ++c) {
              const double w = W.wv(h * HD + j, c);
              o += a.o[c] * w; B += a.A[c] * std::fabs(w); tj += tu[c] * std::fabs(w); pj += pu[c] * std::fabs(w);
            }
            const size_t ix = (size_t)r * d + h * HD + j;
            im.ref[ix] = o + W.bv[h * HD + j];
            im.tol[ix] = 2 * U9 * std::fabs(im.ref[ix]) + tj + pj + kap * (B + std::fabs((double)W.bv[h * HD + j]));
            pert[i][j] = pj;
          }
        });
        bool loose = false;
        for (int r = 0; r < rows; ++r) {
          double mx = 0, pm = 0;
          for (int c = 0; c < d; ++c) mx = std::max(mx, std::fabs(im.ref[(size_t)r * d + c]));
          for (int h = 0; h < H; ++h)
            for (int j = 0; j < HD; ++j) pm = std::max(pm, pert[(size_t)r * H + h][j]);
          if (!(pm <= mx / 16.0)) loose = true;
        }
        if (loose) {
          std::printf("  loose %s: the q' rounding term exceeds 2^-4 of a row's largest |ref|\n", cs.c_str());
          F.result(cs + " (loose)", false, INFINITY);
          continue;
        }
        const Cmp c1 = compare<uint16_t>(im, got);
        F.result(cs + " splits " + std::to_string(S), c1.ok(), c1.w.ratio, c1.str());
      }
  }
  return F.finish();
}

int main(int argc, char** argv) {
  std::string fam = "all";
  for (int i = 1; i < argc; ++i) {
    if (std::string(argv[i]) == "-v") g_verbose = true;
    else fam = argv[i];
  }
  struct Entry { const char* name; int (*fn)(); };
  const Entry table[] = {{"self", fam_self}, {"cross_group", fam_cross_group}, {"cross_capture", fam_cross_capture},
                         {"cross_tf", fam_cross_tf}, {"xq", fam_xq}, {"xattn", fam_xattn}, {"xcomb", fam_xcomb}, {"xchain", fam_xchain}};
  int rc = 0, ran = 0;
  for (const Entry& e : table) {
    if (fam != "all" && fam != e.name) continue;
    g_ref_seconds = 0;
    rc |= e.fn();
    std::printf("  (%s: host reference %.2f s)\n", e.name, g_ref_seconds);
    ++ran;
  }
  if (!ran) {
    std::printf("usage: attn_check self|cross_group|cross_capture|cross_tf|xq|xattn|xcomb|xchain|all [-v]\n");
    return 1;
  }
  return rc;
}
