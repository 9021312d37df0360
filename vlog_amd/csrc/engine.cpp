// libwhisper_mi355 engine: C-ABI (include/whisper_mi355.h) over the gfx950 kernels.
//
// Owns: the packed bf16/f32 weight arena, the encoder scratch, the decoder state (cross-KV slots, self-KV
// cache, token/lineage tables) and the decode loop.  Orchestration mirrors what CTranslate2's
// models::Whisper does below faster-whisper [FW↑] (encode -> generate with logit rules -> results), but the
// loop keeps everything on the device: per step one decoder pass (embed, L x {LN, QKV GEMM -> KV cache,
// self-attn, O GEMM+residual, LN, Q GEMM, cross-attn, O GEMM+residual, LN, FC1+GELU, FC2+residual}, final
// LN, tied-embedding logits GEMM) and one selection kernel; the host only polls an "active hypotheses"
// counter every `check_every` steps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/whisper_mi355.h"
#include "attn.h"
#include "gemm.h"
#include "search.h"
#include "vad.h"

// ---- launchers defined in the .hip files
void launch_logmel(const float*, long long, long long, long long, long long, int, const float*, const float*,
                   const float*, const float*, const int*, const int*, int, float*, long long, unsigned int*, hipStream_t);
void launch_logmel_clamp(float*, long long, long long, long long, const unsigned int*, const float*, hipStream_t);
void launch_ordered_to_float(const unsigned int*, float*, hipStream_t);
void launch_frame_energy(const float*, long long, int, int, float*, hipStream_t);
void launch_pcm_s16(const short*, long long, float*, hipStream_t);
void launch_resample(const void*, int, int, int, long long, long long, long long, const float*, int, int, int, int,
                     long long, long long, float*, hipStream_t);
void launch_layernorm(const float*, long long, const int*, int, int, const float*, const float*, bf16*, long long, hipStream_t);
void launch_embed(const int*, const int*, const bf16*, const float*, float*, int, int, int, int, hipStream_t, int*);
void launch_im2col_conv1(const float*, long long, const int*, const int*, int, int, int, bf16*, hipStream_t);
void launch_zero_pad_rows(bf16*, int, long long, int, hipStream_t);
void launch_attn_enc(const bf16*, bf16*, int, int, int, int, hipStream_t);
// (the decoder attention launchers of attn_dec.hip / attn_xenc.hip: attn.h)

void launch_token_probs(const float*, int, int, int, const int*, float*, hipStream_t);
void launch_align_matrix(const float*, int, int, int, int, int, int, int, float*, float*, float*, hipStream_t);
void launch_align_matrix_batch(const float*, int, int, int, int, int, int, int, int, const int*, const int*, const int*,
                               const long long*, float*, double*, float*, hipStream_t);
void align_set_fused(int on);
int align_get_fused();
void launch_dtw(const float*, int, int, float*, signed char*, int*, int*, int*, hipStream_t);
void launch_dtw_batch(const float*, const long long*, const int*, const int*, float*, signed char*, const long long*,
                      int*, int*, const long long*, int*, int, hipStream_t);
void launch_dtw_open(const float*, int, int, float*, signed char*, int*, int*, int*, int*, hipStream_t);
void launch_dtw_open_batch(const float*, const long long*, const int*, const int*, float*, signed char*, const long long*,
                           int*, int*, const long long*, int*, int*, int, hipStream_t);

// Kernel classes timed by the built-in profiler (wm_profile / wm_profile_read).
enum ProfClass {
  P_LOGMEL = 0, P_ENC_GEMM, P_ENC_ATTN, P_ENC_OTHER, P_CROSSKV_GEMM, P_DEC_GEMM, P_SELF_ATTN, P_CROSS_ATTN,
  P_LOGITS_GEMM, P_SELECT, P_DEC_OTHER, P_CROSS_COMB, P_N
};
static const char* kProfNames[P_N] = {"logmel", "enc_gemm", "enc_attn", "enc_other", "crosskv_gemm", "dec_gemm",
                                      "self_attn", "cross_attn", "logits_gemm", "select", "dec_other", "cross_comb"};

namespace {

thread_local std::string g_err;

#define HIP_OK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e__ = (x);                                                                          \
    if (e__ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e__)); \
  } while (0)

// Bumped whenever a device buffer moves: a captured step graph holds raw pointers, so a decode loop that
// captured one re-captures it when this changed (e.g. a refill pass that grew a scratch buffer).  The counter is
// PER ENGINE: `guarded` points t_realloc at the engine whose entry point runs on this thread (under its lock), so
// another engine's allocations neither force a re-capture nor fail a capture in progress.  Allocations outside an
// entry point (wm_create) count on a fallback no graph reads.
// Greedy row-set compaction threshold in eighths of the pass (VLOG_AMD_COMPACT_8THS, default 7): the live rows are
// packed once they fall to this many eighths of the pass's rows (a step-graph re-capture per compaction).  Variable
// workload, arms alternating on one box: 4/8 2605, 5/8 2644-2645, 6/8 2660-2672, 7/8 2680 RTFx, the same tokens
// (profiles/ab_r05_compact.txt): the cross-attention's items track the live windows more closely, and a re-capture
// costs less than the passes over finished rows it saves.
static int row_compact_8ths() {
  static const int v = [] {
    const char* e = std::getenv("VLOG_AMD_COMPACT_8THS");
    const int x = e ? std::atoi(e) : 7;
    return x >= 1 && x <= 7 ? x : 7;
  }();
  return v;
}

thread_local long long* t_realloc = nullptr;
long long g_realloc_none = 0;
inline long long& realloc_gen() { return t_realloc ? *t_realloc : g_realloc_none; }

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void ensure(size_t b) {
    if (b <= bytes) return;
    if (p) HIP_OK(hipFree(p));
    p = nullptr;
    bytes = 0;
    HIP_OK(hipMalloc(&p, b));
    bytes = b;
    ++realloc_gen();
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T> T* as() const { return (T*)p; }
};

struct Slot {
  size_t off, bytes;
  bool set = false;
  int elem = 2;              // element bytes: 2 = bf16 matrix, 4 = f32 vector / table
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// Decoder projections (index of wm_engine::dec_plan)
enum DecProj { DEC_QKV = 0, DEC_OUT, DEC_CQ, DEC_COUT, DEC_FC1, DEC_FC2, DEC_NPROJ };
static const char* kDecProjNames[DEC_NPROJ] = {"qkv", "out", "cq", "cout", "fc1", "fc2"};
// preset 1 (default): per-projection fastest at 150 rows (tools/dec_gemm_bench, then bench.py A/B).  Round 2:
// fc1 as 64-row x 64-column ring tiles (240 blocks of 320 KB instead of 160 of 480 KB: 12.4 -> 9.0 us) and fc2
// likewise (K split in 4 ranges of 1280, slabs summed by the residual+LayerNorm combine: 16.1 -> 13.8 us with the
// combine); bench.py on one box: dec_gemm 372 -> 352 (fc1) -> 341-343 ms/step (fc2).
static const int kDecPlanPresets[2][DEC_NPROJ] = {{0, -1, -1, -1, 0, -1}, {96, 32, 32, 32, 64, 64}};
static const int kDecColsPresets[2][DEC_NPROJ] = {{32, 32, 32, 32, 32, 32}, {32, 32, 32, 32, 64, 64}};

// Decoder weight pointers per layer (resolved once: the arena layout is fixed at wm_create).
// wm_generate_multilingual: the running call's language state.  The auto windows (h_lang_pos >= 0) were identified
// before generate() runs; their best indices stay on the device (d_top, by auto index) and lang_assign puts the tokens
// into the call's prompt tables before the pass that prefills them.
struct LangCall {
  int lang_begin = 0, n_langs = 0;
  std::vector<int> pos, aidx;     // [n_windows]: the language position (-1: the window keeps its prompt), the auto index
  const int* d_top = nullptr;     // [auto windows]
  std::vector<int> h_ent;         // host image of a row-set event's entry list (alive until the next poll synchronises)
};

struct DecLayerW {
  const bf16 *qkv_w, *out_w, *cq_w, *cout_w, *fc1_w, *fc2_w;
  const float *qkv_b, *out_b, *cq_b, *cout_b, *fc1_b, *fc2_b, *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ln3_w, *ln3_b;
};

struct wm_engine {
  wm_model_dims dm;
  int device;
  std::mutex mu;
  bool weights_ok = false;     // every weight slot set (cached by require_weights)
  long long realloc_gen = 0;   // this engine's buffer generation (t_realloc while one of its entry points runs)
  // weights
  std::map<std::string, Slot> slots;
  std::vector<std::string> slot_order;   // weight names in layout order (wm_weight_info)
  DevBuf arena;
  int k1p;  // padded conv1 K
  // frontend constants
  DevBuf fe_window, fe_cos, fe_sin, fe_filt, fe_lo, fe_hi;
  // encoder scratch
  DevBuf e_cols, e_h1, e_x, e_hb, e_qkv, e_ao, e_ff, e_seek, e_len;
  int enc_cap = 0;
  int enc_chunk = 160;       // windows per encoder pass (activation scratch ~52 MB per large-v3 window; bigger
                             // passes cut the GEMM tail rounds: 16 -> 150 measured +1.2 % end to end)
  // decoder state
  int n_slots = 0, n_hyp_cap = 0;
  DevBuf ckv, skv;
  DevBuf d_tokens, d_lin, d_seq_len, d_done, d_cum, d_row_tok, d_row_pos, d_row_hyp, d_hyp_slot, d_n_active;
  DevBuf d_suppress, d_cand_tok, d_cand_lp, d_fin_tok, d_fin_len, d_fin_cum, d_n_fin, d_ns, d_logit_rows;
  DevBuf d_prow_tok, d_prow_pos, d_prow_hyp, d_head_map;
  // d_n_active holds [0] the live-hypothesis counter and [1..3] the decode's device error word (common.h
  // wm_report_error), so one poll copy reads both
  // per-step records (wm_generate_args h_token_logprobs): per hypothesis, per finished beam candidate
  DevBuf d_tok_lp, d_tok_lp_o, d_fin_lp;
  // row-set decode (generate_rows): per-window prompts / slots, slot -> output id, output tables by window, and
  // the event upload (pass rows, row set, logit rows, starts)
  DevBuf d_win_prompt, d_win_slot, d_hyp_out, d_res_tok, d_res_len, d_res_cum, d_res_ns, d_res_lp, d_res_lp_o, d_ev;
  DevBuf d_hyp_begin, d_hyp_maxlen, d_win_len, d_win_maxlen;   // ragged prompts (search.h hyp_begin / hyp_maxlen)
  // per-window seeds (wm_generate_seeded; search.h hyp_seed / hyp_key): the running call's host seeds [n_windows]
  // (nullptr outside such a call) and the device tables
  const uint64_t* call_seeds = nullptr;
  // wm_generate_multilingual: the running call's language state (nullptr outside such a call), its device tables
  // ([4] error word | [n] top | [n] top probability | [n][n_langs] probabilities) and lang_assign's entry list
  LangCall* call_lang = nullptr;
  DevBuf d_la, d_la_ent;
  // ... and the pinned host image of d_la: its copy back is queued behind the language head and has arrived when
  // generate()'s own final synchronise returns (pinned, so the copy is asynchronous to the host)
  void* h_la = nullptr;
  size_t h_la_bytes = 0;
  DevBuf d_hyp_seed, d_hyp_key, d_win_seed;
  std::vector<int> h_ev;     // host image of d_ev (kept alive until the next poll syncs the stream)
  // sequence-bias table (wm_set_sequence_bias; search.h bias_*): allocated once at the limits' size, so a captured
  // step graph's pointers stay valid whatever table follows
  DevBuf d_sb_off, d_sb_tok, d_sb_val;
  int n_seq_bias = 0;
  int dbg_nan_row = -1;      // TEST ONLY (wm_set_option "debug_nan_row"): NaN logits row before every selection
  int dbg_nan_count = 1;     // TEST ONLY ("debug_nan_count"): rows [debug_nan_row, + count) (a whole beam group: nlive 0)
  // step activations
  DevBuf s_x, s_hb, s_q, s_ao, s_ff, s_logits, s_pm, s_pl, s_po;
  // profiler: per class, HIP event pairs recorded on the launch stream + algorithmic flops / bytes
  bool prof_on = false;
  unsigned prof_mask = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[P_N];
  std::vector<hipEvent_t> ev_pool;
  double prof_flops[P_N] = {0}, prof_bytes[P_N] = {0};
  DevBuf gemm_ws, gemm_ws2;  // split-K partial slabs (per decoder slice stream)
  // two-slice decode (decoder_pass): second stream + fork/phase/join events
  bool dec_ring = true;      // ring-pipelined decoder GEMMs for the wide K <= 1280 projections (gemm_dec.hip)
  // Decoder projection plan, per projection (DEC_QKV .. DEC_FC2), for passes of <= 1024 rows:
  //   > 0  ring GEMM with the rows in groups of that many (one block per 32-column tile x row group x K split)
  //     0  ring GEMM, all rows in one block (passes of <= 160 rows; wide projections only)
  //    -1  skinny split-K GEMM (gemm.hip launch_gemm)
  //    -2  one-shot GEMM (gemm_dec.hip launch_dec_oneshot)
  // Preset 1 (default) is the fastest per projection measured at 150 rows (tools/dec_gemm_bench);
  // preset 0 is round 1's routing.
  int dec_plan[6] = {96, 32, 32, 32, 64, 64};
  int dec_cols[6] = {32, 32, 32, 32, 64, 64};   // ring GEMM output columns per block (32 or 64)
  int dec_kr[6] = {0, 0, 0, 0, 0, 0};           // ring GEMM K range per block (0: the whole K up to 1280)
  bool dec_split = false;    // two-stream row slices (see decoder_pass)
  int dec_graph = 1;         // decode steps replayed from one captured HIP graph (see generate)
  int dec_gemv = 1;          // passes of <= 32 rows: the small-M weight-streaming GEMM (gemm_dec.hip gemv)
  int dec_gemv_ln = 1;       // passes of <= 16 rows: the LayerNorms after out / cout computed inside cq / fc1
  int dec_gemv_ln_fc2 = 0;   // ... and the one after fc2 inside the next layer's qkv (fc2 a 16-wave residual producer):
                             // measured slower (fc2 on 80 blocks 11.5 us alone, as slab + combine; qkv +2.4 us)
  DevBuf d_lnstat;           // their per-(tile, row) partial row sums, one region per decode slice
  hipStream_t gst = nullptr; // the capture / replay stream (a graph cannot be captured on the legacy null stream)
  hipEvent_t ev_g0 = nullptr, ev_g1 = nullptr;
  int cross_fuse = 1;        // bit 0: cq split-K combine, bit 1: key-split combine (last arriver), folded into
                             // the cross-attention kernel; bit 1 measured slower (per-item hand-off latency)
  DevBuf d_cross_cnt;        // its per-(row, head) arrival counters (zeroed at allocation, reset in-kernel)
  // cross-attention form: 1 = factored (attention over the encoder output, attn_xenc.hip: a window's slot
  // holds its encoder output, 3.84 MB for large-v3), 0 = projected cross-KV panels (attn_dec.hip: 245.8 MB
  // per large-v3 window, projected by wm_cross_kv)
  int cross_mode = 1;
  int cross_tf = 1;          // teacher-forced passes (alignment) run the projected form's cross-attention on MFMA
  int cross_mfma = 1;        // projected form, decode passes with 2..32 rows per window (beam groups): MFMA kernel
  int cross_mfma_fuse = 0;   // ... its key-split combine done by the last-arriving split (d_cross_cnt), not a kernel:
                             // measured slower (16.3 vs 15.3 us per layer at 1 window, beam 5: the L2 hand-off
                             // costs ~3 round trips, more than the combine kernel behind it in the stream)
  int dec_big_rows = 161;    // passes of >= this many rows (beam groups of many windows): 64-row ring groups, the
                             // whole K per block (decoder_layer); 320 before the two-blocks-per-CU tiles below
  int dec_big128 = 512;      // ... from this many rows the 8-wave ring plan (0: never; VLOG_AMD_DEC_BIG128): qkv, fc1
                             // and fc2 as 128 x 128 tiles (fc2's K of 4d in ranges of dec_big_fc2_kr), the d x d
                             // projections as 64 x 64 tiles, one block of 8 waves per CU.  Config 5 (750 rows): dec_gemm
                             // 568 -> 504-506 ms per step, same tokens (profiles/ab_r06_c5_plan*.txt).  Below 512 rows
                             // the 4-wave 64-row groups stay (tools/dec_gemm_bench at 384 rows, profiles/dgb_r06_*).
  int dec_big_fc2_kr = 1280; // ... fc2's K range per block on that plan (0: the whole K; 1280: four ranges, 240 blocks,
                             // slabs summed by its residual + LayerNorm combine; whole K = 60 blocks, 50 us in the step)
  int dec_big_lds = 72;      // ... qkv / fc1 / fc2 with this LDS budget per ring block (KiB): 72 = two resident blocks
                             // per CU (tools/dec_gemm_bench at 750 rows: qkv 24.7 -> 18.8 us, fc1 31.3 -> 21.4, fc2
                             // 41.6 -> 33.1 against 144; at 256 rows qkv+fc1+fc2 45.6 -> 35.7 us per layer against the
                             // 150-row plan; bit-identical: the ring depth never changes a row's K order)
  int xkeep = 0;             // factored cross-attention: window groups whose encoder output is loaded with the default
                             // cache policy (the rest non-temporal), to keep them in the Infinity Cache across layers
  bool xsnake = false;       // factored cross-attention: odd layers walk each XCD's items in reverse (Infinity Cache reuse)
  DevBuf xenc;               // factored: [n_slots][T][d] bf16 encoder outputs (cross_fp8: OCP e4m3 bytes)
  DevBuf xscale;             // cross_fp8: [n_slots][T] f32 per-position scales
  int cross_fp8 = 0;         // opt-in fp8 cross memory (factored form only; changes numerics, never the default)
  // opt-in fp8 K/V panels of the PROJECTED form (independent of cross_fp8; changes numerics, never the default):
  //   0  bf16 panels in ckv
  //   1  ckv holds e4m3 codes [L][2][n_slots][H][T][64] bytes, ckv_exp one exponent byte per 64-code row
  //      [L][2][n_slots][H][T]; the attention kernels' F8 instantiations convert on load (attn_dec.hip)
  //   2  reference form: bf16 panels holding the dequantised values of form 1, read by the bf16 kernels
  // Forms 1 and 2: wm_cross_kv projects KV8_STAGE_WINDOWS windows at a time into kv8_stage (bf16, panel layout) and
  // the quantiser writes their slots.
  int cross_kv_fp8 = 0;
  DevBuf ckv_exp, kv8_stage;
  static constexpr int KV8_STAGE_WINDOWS = 2;   // at most 2 x 245.8 MB = 491.5 MB of staging at large-v3 (a call of
                                                // one window stages one)
  DevBuf xwkt;               // factored: Wk^T per layer and head [L][H][d][64] bf16, packed from dec.ckv.w
  DevBuf xwvb;               // factored: Wv per layer and head in 16-column blocks [L][H][d/16][64][16]
  bool xwkt_ready = false;
  DevBuf s_qp, s_pu, s_pml;  // factored step scratch: q' [rows][H][d], split partials u/l and (m, l)
  int cross_cap = 0;         // cross-attention grid cap (0: one block per item; >0: persistent grid-stride form,
                             // 2 blocks/CU measured ~2 % faster alone but slower with the fused q combine)
  hipStream_t st2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_mid = nullptr, ev_join = nullptr;
  std::vector<DecLayerW> dec_w;
  // factored form, teacher-forced alignment pass: the pass's windows' encoder outputs gathered contiguously, and one
  // layer's projected K/V panels of them [2][tf_nwin][H][T][64] (re-projected per layer on MFMA)
  DevBuf a_enc, a_kv;
  int tf_nwin = 0;
  DevBuf a_logits, a_attn, a_next, a_probs, a_rowsum, a_z, a_mat, a_cost, a_trace, a_pi, a_pj, a_plen, a_meta;
  DevBuf prof_dbytes;        // device counters (attention kernels add the bytes they actually read)
  // wm_resample: per ratio (up, down), the f32 taps in polyphase order [up][T] on the device (built once)
  struct RsTaps {
    int T = 0;
    DevBuf pp;
  };
  std::map<std::pair<int, int>, RsTaps> rs_taps;
  hipEvent_t ev_get() {
    if (ev_pool.empty()) {
      hipEvent_t ev;
      HIP_OK(hipEventCreate(&ev));
      return ev;
    }
    hipEvent_t ev = ev_pool.back();
    ev_pool.pop_back();
    return ev;
  }
  unsigned long long* dstat(int cls) { return (prof_on && ((prof_mask >> cls) & 1u)) ? prof_dbytes.as<unsigned long long>() + (size_t)cls * STAT_SLOTS : nullptr; }

  const Slot& slot(const std::string& n) const {
    auto it = slots.find(n);
    if (it == slots.end()) throw std::runtime_error("unknown weight " + n);
    return it->second;
  }
  template <class T> T* W(const std::string& n) const { return (T*)((char*)arena.p + slot(n).off); }
  const bf16* Wb(const std::string& n) const { return W<bf16>(n); }
  const float* Wf(const std::string& n) const { return W<float>(n); }

  size_t device_bytes() const {
    size_t t = arena.bytes;
    for (const DevBuf* b : {&e_cols, &e_h1, &e_x, &e_hb, &e_qkv, &e_ao, &e_ff, &ckv, &ckv_exp, &kv8_stage, &xenc, &xscale, &xwkt, &xwvb, &s_qp, &s_pu, &skv, &s_x, &s_hb, &s_q, &s_ao,
                            &s_ff, &s_logits, &s_pm, &s_pl, &s_po, &d_tokens, &d_lin, &d_fin_tok})
      t += b->bytes;
    return t;
  }
};

namespace {

void add_slot(wm_engine* e, size_t& off, const std::string& name, size_t count, int elem) {
  e->slots[name] = Slot{off, count * elem, false, elem};
  e->slot_order.push_back(name);
  off += align256(count * elem);
}

void build_layout(wm_engine* e) {
  const auto& m = e->dm;
  const size_t d = m.n_state, f = 4 * d, b2 = 2, f4 = 4;
  e->k1p = ((3 * m.n_mels + 63) / 64) * 64;
  size_t off = 0;
  add_slot(e, off, "enc.conv1.w", d * e->k1p, 2);
  add_slot(e, off, "enc.conv1.b", d, 4);
  add_slot(e, off, "enc.conv2.w", d * 3 * d, 2);
  add_slot(e, off, "enc.conv2.b", d, 4);
  add_slot(e, off, "enc.pos", (size_t)m.n_audio_ctx * d, 4);
  for (int l = 0; l < m.n_enc_layer; ++l) {
    const std::string p = "enc." + std::to_string(l) + ".";
    add_slot(e, off, p + "ln1.w", d, 4); add_slot(e, off, p + "ln1.b", d, 4);
    add_slot(e, off, p + "qkv.w", 3 * d * d, 2); add_slot(e, off, p + "qkv.b", 3 * d, 4);
    add_slot(e, off, p + "out.w", d * d, 2); add_slot(e, off, p + "out.b", d, 4);
    add_slot(e, off, p + "ln2.w", d, 4); add_slot(e, off, p + "ln2.b", d, 4);
    add_slot(e, off, p + "fc1.w", f * d, 2); add_slot(e, off, p + "fc1.b", f, 4);
    add_slot(e, off, p + "fc2.w", d * f, 2); add_slot(e, off, p + "fc2.b", d, 4);
  }
  add_slot(e, off, "enc.ln.w", d, 4); add_slot(e, off, "enc.ln.b", d, 4);
  add_slot(e, off, "dec.embed", (size_t)m.n_vocab * d, 2);
  add_slot(e, off, "dec.pos", (size_t)m.n_text_ctx * d, 4);
  for (int l = 0; l < m.n_dec_layer; ++l) {
    const std::string p = "dec." + std::to_string(l) + ".";
    add_slot(e, off, p + "ln1.w", d, 4); add_slot(e, off, p + "ln1.b", d, 4);
    add_slot(e, off, p + "qkv.w", 3 * d * d, 2); add_slot(e, off, p + "qkv.b", 3 * d, 4);
    add_slot(e, off, p + "out.w", d * d, 2); add_slot(e, off, p + "out.b", d, 4);
    add_slot(e, off, p + "ln2.w", d, 4); add_slot(e, off, p + "ln2.b", d, 4);
    add_slot(e, off, p + "cq.w", d * d, 2); add_slot(e, off, p + "cq.b", d, 4);
    add_slot(e, off, p + "cout.w", d * d, 2); add_slot(e, off, p + "cout.b", d, 4);
    add_slot(e, off, p + "ln3.w", d, 4); add_slot(e, off, p + "ln3.b", d, 4);
    add_slot(e, off, p + "fc1.w", f * d, 2); add_slot(e, off, p + "fc1.b", f, 4);
    add_slot(e, off, p + "fc2.w", d * f, 2); add_slot(e, off, p + "fc2.b", d, 4);
  }
  add_slot(e, off, "dec.ckv.w", (size_t)m.n_dec_layer * 2 * d * d, 2);
  add_slot(e, off, "dec.ckv.b", (size_t)m.n_dec_layer * 2 * d, 4);
  add_slot(e, off, "dec.ln.w", d, 4); add_slot(e, off, "dec.ln.b", d, 4);
  e->arena.ensure(off);
}

// slaney mel filterbank (faster-whisper get_mel_filters), periodic Hann, DFT twiddles — host f64 -> f32
void build_frontend(wm_engine* e, hipStream_t st) {
  const int nm = e->dm.n_mels, nb = 201, nfft = 400, sr = 16000;
  std::vector<float> win(nfft), c(nfft), s(nfft);
  for (int n = 0; n < nfft; ++n) {
    win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / nfft));
    c[n] = (float)std::cos(2.0 * M_PI * n / nfft);
    s[n] = (float)std::sin(2.0 * M_PI * n / nfft);
  }
  std::vector<double> mels(nm + 2), freqs(nm + 2), fft(nb);
  const double max_mel = 45.245640471924965, f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
  const double logstep = std::log(6.4) / 27.0;
  for (int i = 0; i < nm + 2; ++i) {
    mels[i] = max_mel * i / (nm + 1);
    freqs[i] = mels[i] >= min_log_mel ? min_log_hz * std::exp(logstep * (mels[i] - min_log_mel)) : f_sp * mels[i];
  }
  for (int k = 0; k < nb; ++k) fft[k] = (double)k * sr / nfft;
  std::vector<float> filt((size_t)nm * nb, 0.f);
  std::vector<int> lo(nm, nb), hi(nm, 0);
  for (int m = 0; m < nm; ++m) {
    const double enorm = 2.0 / (freqs[m + 2] - freqs[m]);
    for (int k = 0; k < nb; ++k) {
      const double lower = -(freqs[m] - fft[k]) / (freqs[m + 1] - freqs[m]);
      const double upper = (freqs[m + 2] - fft[k]) / (freqs[m + 2] - freqs[m + 1]);
      const double w = std::max(0.0, std::min(lower, upper)) * enorm;
      filt[(size_t)m * nb + k] = (float)w;
      if (w > 0) { lo[m] = std::min(lo[m], k); hi[m] = std::max(hi[m], k + 1); }
    }
    if (lo[m] >= hi[m]) { lo[m] = 0; hi[m] = 0; }
  }
  auto up = [&](DevBuf& b, const void* src, size_t bytes) {
    b.ensure(bytes);
    HIP_OK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
  };
  up(e->fe_window, win.data(), nfft * 4);
  up(e->fe_cos, c.data(), nfft * 4);
  up(e->fe_sin, s.data(), nfft * 4);
  up(e->fe_filt, filt.data(), filt.size() * 4);
  up(e->fe_lo, lo.data(), nm * 4);
  up(e->fe_hi, hi.data(), nm * 4);
  HIP_OK(hipStreamSynchronize(st));
}

GemmEpi epi_of(int kind, void* out, long long ldc, const float* bias) {
  GemmEpi p;
  std::memset(&p, 0, sizeof(p));
  p.kind = kind;
  p.out = out;
  p.ldc = ldc;
  p.bias = bias;
  return p;
}
GemmA amat(const bf16* ptr, long long ld) { return GemmA{ptr, ld, 0, 0}; }

// Times one kernel class.  Plain mode records events around the launches; `attached` mode hands the two
// events to a launcher that attaches them to the dispatch itself (hipExtLaunchKernelGGL), which times the
// kernel alone (what rocprofv3 reports) instead of kernel + event-record overhead.
struct ProfScope {
  wm_engine* e;
  int cls;
  hipStream_t st;
  bool attached;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(wm_engine* e_, int cls_, hipStream_t st_, double flops = 0, double bytes = 0, bool attached_ = false)
      : e(e_), cls(cls_), st(st_), attached(attached_) {
    if (!e->prof_on || !((e->prof_mask >> cls) & 1u)) return;
    a = e->ev_get();
    b = e->ev_get();
    if (!attached) HIP_OK(hipEventRecord(a, st));
    e->prof_flops[cls] += flops;
    e->prof_bytes[cls] += bytes;
  }
  ~ProfScope() {
    if (!a) return;
    if (!attached) (void)hipEventRecord(b, st);
    e->prof_ev[cls].push_back({a, b});
  }
};

// algorithmic bytes of a GEMM: A (M x K bf16) + W (N x K bf16) + output
double gemm_bytes(double M, double N, double K, double out_bytes) { return 2 * M * K + 2 * N * K + out_bytes * M * N; }

void gemm_p(wm_engine* e, int cls, const GemmA& a, const bf16* w, long long ldw, int M, int N, int K, const GemmEpi& ep,
            hipStream_t st) {
  const double ob = (ep.kind == EPI_RESID_F32) ? 8 : (ep.kind == EPI_RESID_LN) ? 10 : (ep.kind == EPI_F32 || ep.kind == EPI_GELU_POS_F32) ? 4 : 2;
  ProfScope ps(e, cls, st, 2.0 * M * N * K, gemm_bytes(M, N, K, ob));
  // split-K only where the grid is too small to fill the chip (decoder rows); 64 MB slab scratch
  const size_t wsb = 64ull << 20;
  e->gemm_ws.ensure(wsb);
  launch_gemm(a, w, ldw, M, N, K, ep, e->gemm_ws.as<float>(), wsb, st);
}

// ------------------------------------------------------------------------------------------ encoder
void encode_chunk(wm_engine* e, const float* mel, long long ld, const int* h_seek, const int* h_len, int B, bf16* out,
                  hipStream_t st) {
  const auto& m = e->dm;
  const int d = m.n_state, T = m.n_audio_ctx, L = m.n_enc_layer, H = m.n_head;
  const long long M = (long long)B * T;
  if (B > e->enc_cap) {
    e->e_cols.ensure((size_t)B * 3000 * e->k1p * 2);
    e->e_h1.ensure((size_t)B * 3001 * d * 2);
    e->e_x.ensure((size_t)M * d * 4);
    e->e_hb.ensure((size_t)M * d * 2);
    e->e_qkv.ensure((size_t)M * 3 * d * 2);
    e->e_ao.ensure((size_t)M * d * 2);
    e->e_ff.ensure((size_t)M * 4 * d * 2);
    e->e_seek.ensure(B * 4);
    e->e_len.ensure(B * 4);
    e->enc_cap = B;
  }
  HIP_OK(hipMemcpyAsync(e->e_seek.p, h_seek, B * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->e_len.p, h_len, B * 4, hipMemcpyHostToDevice, st));
  bf16* cols = e->e_cols.as<bf16>();
  bf16* h1 = e->e_h1.as<bf16>();
  float* x = e->e_x.as<float>();
  bf16* hb = e->e_hb.as<bf16>();
  bf16* qkv = e->e_qkv.as<bf16>();
  bf16* ao = e->e_ao.as<bf16>();
  bf16* ff = e->e_ff.as<bf16>();
  // conv1 (implicit GEMM over the window-sliced mel) + GELU -> h1 rows 1..3000 of each [3001][d] block
  {
    ProfScope ps(e, P_ENC_OTHER, st);
    launch_im2col_conv1(mel, ld, e->e_seek.as<int>(), e->e_len.as<int>(), B, m.n_mels, e->k1p, cols, st);
    launch_zero_pad_rows(h1, B, 3001LL * d, d, st);
  }
  {
    GemmEpi ep = epi_of(EPI_BF16, h1, d, e->Wf("enc.conv1.b"));
    ep.act = 1; ep.rpb = 3000; ep.bstride = 3001LL * d; ep.roff = 1;
    gemm_p(e, P_ENC_GEMM, amat(cols, e->k1p), e->Wb("enc.conv1.w"), e->k1p, B * 3000, d, e->k1p, ep, st);
  }
  // conv2 (k3, s2): row t of window b reads h1 rows 2t-1, 2t, 2t+1 = 3d contiguous elements starting at
  // block row 2t (the zero row 0 is the left padding); + GELU + positional embedding -> residual x
  {
    GemmA a{h1, 2LL * d, T, 3001LL * d};
    GemmEpi ep = epi_of(EPI_GELU_POS_F32, x, d, e->Wf("enc.conv2.b"));
    ep.rpb = T; ep.pos = e->Wf("enc.pos");
    gemm_p(e, P_ENC_GEMM, a, e->Wb("enc.conv2.w"), 3LL * d, (int)M, d, 3 * d, ep, st);
  }
  for (int l = 0; l < L; ++l) {
    const std::string p = "enc." + std::to_string(l) + ".";
    {
      ProfScope ps(e, P_ENC_OTHER, st);
      launch_layernorm(x, d, nullptr, (int)M, d, e->Wf(p + "ln1.w"), e->Wf(p + "ln1.b"), hb, d, st);
    }
    gemm_p(e, P_ENC_GEMM, amat(hb, d), e->Wb(p + "qkv.w"), d, (int)M, 3 * d, d, epi_of(EPI_BF16, qkv, 3LL * d, e->Wf(p + "qkv.b")), st);
    {
      ProfScope ps(e, P_ENC_ATTN, st, 4.0 * B * (double)T * T * d, 2.0 * 4 * M * d);
      launch_attn_enc(qkv, ao, B, T, d, H, st);
    }
    gemm_p(e, P_ENC_GEMM, amat(ao, d), e->Wb(p + "out.w"), d, (int)M, d, d, epi_of(EPI_RESID_F32, x, d, e->Wf(p + "out.b")), st);
    {
      ProfScope ps(e, P_ENC_OTHER, st);
      launch_layernorm(x, d, nullptr, (int)M, d, e->Wf(p + "ln2.w"), e->Wf(p + "ln2.b"), hb, d, st);
    }
    {
      GemmEpi ep = epi_of(EPI_BF16, ff, 4LL * d, e->Wf(p + "fc1.b"));
      ep.act = 1;
      gemm_p(e, P_ENC_GEMM, amat(hb, d), e->Wb(p + "fc1.w"), d, (int)M, 4 * d, d, ep, st);
    }
    gemm_p(e, P_ENC_GEMM, amat(ff, 4LL * d), e->Wb(p + "fc2.w"), 4LL * d, (int)M, d, 4 * d, epi_of(EPI_RESID_F32, x, d, e->Wf(p + "fc2.b")), st);
  }
  ProfScope ps(e, P_ENC_OTHER, st);
  launch_layernorm(x, d, nullptr, (int)M, d, e->Wf("enc.ln.w"), e->Wf("enc.ln.b"), out, d, st);
}

// ------------------------------------------------------------------------------------------ decoder
void ensure_step(wm_engine* e, int rows, int logit_rows) {
  const int d = e->dm.n_state, H = e->dm.n_head;
  e->s_x.ensure((size_t)rows * d * 4);
  e->s_hb.ensure((size_t)rows * d * 2);
  e->s_q.ensure((size_t)rows * d * 2);
  e->s_ao.ensure((size_t)rows * d * 2);
  e->s_ff.ensure((size_t)rows * 4 * d * 2);
  e->s_logits.ensure((size_t)logit_rows * e->dm.n_vocab * 4);
  e->s_pm.ensure((size_t)rows * H * 16 * 4);
  e->s_pl.ensure((size_t)rows * H * 16 * 4);
  e->s_po.ensure((size_t)rows * H * 16 * 64 * 4);
  if (e->d_cross_cnt.bytes < (size_t)rows * H * 4) {
    e->d_cross_cnt.ensure((size_t)rows * H * 4);
    HIP_OK(hipMemset(e->d_cross_cnt.p, 0, e->d_cross_cnt.bytes));
  }
  e->d_prow_tok.ensure((size_t)rows * 4);
  e->d_prow_pos.ensure((size_t)rows * 4);
  e->d_prow_hyp.ensure((size_t)rows * 4);
  e->d_logit_rows.ensure((size_t)logit_rows * 4);
}

const std::vector<DecLayerW>& dec_weights(wm_engine* e) {
  if ((int)e->dec_w.size() == e->dm.n_dec_layer) return e->dec_w;
  e->dec_w.clear();
  for (int l = 0; l < e->dm.n_dec_layer; ++l) {
    const std::string p = "dec." + std::to_string(l) + ".";
    DecLayerW w;
    w.qkv_w = e->Wb(p + "qkv.w"); w.out_w = e->Wb(p + "out.w"); w.cq_w = e->Wb(p + "cq.w");
    w.cout_w = e->Wb(p + "cout.w"); w.fc1_w = e->Wb(p + "fc1.w"); w.fc2_w = e->Wb(p + "fc2.w");
    w.qkv_b = e->Wf(p + "qkv.b"); w.out_b = e->Wf(p + "out.b"); w.cq_b = e->Wf(p + "cq.b");
    w.cout_b = e->Wf(p + "cout.b"); w.fc1_b = e->Wf(p + "fc1.b"); w.fc2_b = e->Wf(p + "fc2.b");
    w.ln1_w = e->Wf(p + "ln1.w"); w.ln1_b = e->Wf(p + "ln1.b"); w.ln2_w = e->Wf(p + "ln2.w");
    w.ln2_b = e->Wf(p + "ln2.b"); w.ln3_w = e->Wf(p + "ln3.w"); w.ln3_b = e->Wf(p + "ln3.b");
    e->dec_w.push_back(w);
  }
  return e->dec_w;
}

// A contiguous range of decoder rows [r0, r0 + rows) of a pass over total_rows, issued on its own stream
// with its own split-K scratch.
struct DecSlice {
  int r0, rows, total_rows;
  hipStream_t st;
  DevBuf* ws;
};

// Issues decoder layer l for one slice.  `mid` (optional) is recorded on the slice's stream right before its
// cross-attention, which is where the second slice starts (see decoder_pass).
void decoder_layer(wm_engine* e, const DecSlice& sl, int l, const int* row_pos, const int* row_hyp, const int* done,
                   const int* lin, const std::vector<std::vector<int>>* align_map, int n_align, float* attn,
                   int cross_group, hipEvent_t mid) {
  const auto& m = e->dm;
  const int d = m.n_state, H = m.n_head, L = m.n_dec_layer, T = m.n_audio_ctx, C = m.n_text_ctx;
  const int r0 = sl.r0, rows = sl.rows;
  hipStream_t st = sl.st;
  float* x = e->s_x.as<float>() + (size_t)r0 * d;
  bf16* hb = e->s_hb.as<bf16>() + (size_t)r0 * d;
  bf16* q = e->s_q.as<bf16>() + (size_t)r0 * d;
  bf16* ao = e->s_ao.as<bf16>() + (size_t)r0 * d;
  bf16* ff = e->s_ff.as<bf16>() + (size_t)r0 * 4 * d;
  row_pos += r0;
  row_hyp += r0;
  const size_t skv_layer = (size_t)e->n_hyp_cap * H * C * 64;      // elements per (layer, k|v)
  const size_t ckv_layer = (size_t)e->n_slots * H * T * 64;
  bf16* skv = e->skv.as<bf16>();
  bf16* ckv = e->ckv.as<bf16>();
  const size_t cexp_layer = (size_t)e->n_slots * H * T;            // fp8 panels: exponent bytes per (layer, k|v)
  const auto& W = dec_weights(e)[l];
  const size_t wsb = 64ull << 20;
  sl.ws->ensure(wsb);
  float* ws = sl.ws->as<float>();
  // The route of each projection follows the whole pass's rows (sl.total_rows), so slicing a pass never changes
  // a row's arithmetic.  Long prefills (> 1024 rows) keep the large-tile GEMMs.
  auto plan_of = [&](int proj) -> int { return sl.total_rows > 1024 ? -1 : e->dec_plan[proj]; };
  auto gemm = [&](int proj, const GemmA& a, const bf16* w, long long ldw, int N, int K, const GemmEpi& ep) {
    const double ob = (ep.kind == EPI_RESID_F32) ? 8 : (ep.kind == EPI_RESID_LN) ? 10 : 2;
    ProfScope ps(e, P_DEC_GEMM, st, 2.0 * rows * N * K, gemm_bytes(rows, N, K, ob));
    // one window's beam (or a handful of rows): the weight-streaming small-M kernel
    if (sl.total_rows <= 32 && e->dec_gemv && launch_dec_gemv(a, w, ldw, rows, N, K, ep, ws, wsb, st)) return;
    if (a.lnx || ep.stat_out) throw std::runtime_error("decoder: fused LayerNorm operand off the small-M path");
    // passes of >= dec_big_rows rows (beam groups of many windows; tools/dec_gemm_bench at 384 and 750 rows): 64-row
    // ring groups; 64 columns for qkv and fc1, and for every projection from 512 rows; fc2's whole K per block
    // (384 rows: 76 vs 86 us per layer for the 150-row plan; 750 rows: 114 vs 159 us)
    const int tr = sl.total_rows;
    const bool big = e->dec_big_rows > 0 && tr >= e->dec_big_rows && tr <= 1024;
    // (dec_big128 from round 6: the 8-wave plan below; round 4's form, qkv / fc1 / fc2 in 4-wave 128-row groups,
    // two blocks per CU at 750 rows: 17.2 / 18.4 / 25.6 us against
    // 18.9 / 21.0 / 32.8 for 64-row groups in tools/dec_gemm_bench, yet slower inside the decode step)
    const bool sq = proj == DEC_OUT || proj == DEC_CQ || proj == DEC_COUT;
    const bool b128 = big && e->dec_big128 > 0 && tr >= e->dec_big128;
    int p = big ? 64 : plan_of(proj);
    // the three d x d projections keep 32-column tiles below 512 rows and one block per CU (144 KiB); qkv / fc1 / fc2
    // take 64 x 64 tiles, two blocks per CU (dec_big_lds; tools/dec_gemm_bench at 256 / 384 / 750 rows,
    // profiles/dec_gemm_bench_r04_*rows_lds*.txt)
    int cols = big ? ((tr >= 512 || !sq) ? 64 : 32) : e->dec_cols[proj];
    int lds = big ? (sq ? 144 : e->dec_big_lds) : 0;
    int waves = 4;
    int kr_big = 0;
    if (b128) {                            // the 8-wave plan (dec_big128)
      if (sq) { p = 64; cols = 64; lds = 144; waves = 8; }
      else { p = 128; cols = 128; lds = 144; waves = 8; }
      // fc2 (K = 4d) in K ranges of dec_big_fc2_kr: as 128 x 128 tiles over the whole K (60 blocks) it took 50 us per
      // launch in the step against 27.5 for the 4-wave 64 x 64 tiles (rocprof, config 5), though 25 us in
      // tools/dec_gemm_bench: a block streams its 1.3 MB activation panel from the MALL at the per-CU rate, so few
      // blocks lose in the step.  Qkv 128 x 64 (two blocks per CU) / fc1 128 x 64 / fc2 128 x 64 in two K ranges
      // measured 5 / 2 / 10 ms per step slower (profiles/ab_r06_c5_plan2.txt)
      if (proj == DEC_FC2) kr_big = e->dec_big_fc2_kr;
      // VLOG_AMD_DEC_BIG_<QKV|SQ|FC1|FC2>="rows,cols,lds,kr,waves" overrides a projection's plan (A/B only)
      static const int* const ov = [] {
        static int v[4][5] = {};
        const char* names[4] = {"VLOG_AMD_DEC_BIG_QKV", "VLOG_AMD_DEC_BIG_SQ", "VLOG_AMD_DEC_BIG_FC1", "VLOG_AMD_DEC_BIG_FC2"};
        for (int i = 0; i < 4; ++i)
          if (const char* ev = std::getenv(names[i]))
            if (std::sscanf(ev, "%d,%d,%d,%d,%d", &v[i][0], &v[i][1], &v[i][2], &v[i][3], &v[i][4]) != 5) v[i][0] = 0;
        return &v[0][0];
      }();
      const int* o = ov + 5 * (sq ? 1 : proj == DEC_QKV ? 0 : proj == DEC_FC1 ? 2 : 3);
      if (o[0] > 0) { p = o[0]; cols = o[1]; lds = o[2]; kr_big = o[3]; waves = o[4]; }
    }
    if (p == -2 && launch_dec_oneshot(a, w, ldw, rows, N, K, ep, ws, wsb, N >= 3 * K ? 4 : 2, st)) return;
    // ring: one pass over each 1280-deep K range, epilogue in place (K > 1280: slabs summed by the combine)
    const int kr = kr_big > 0 ? std::min(kr_big, K) : e->dec_kr[proj] > 0 ? std::min(e->dec_kr[proj], K) : (K <= 1280 || big ? K : 1280);
    if (p > 0 && launch_dec_ring(a, w, ldw, rows, N, K, ep, ws, wsb, kr, st, p, cols, lds, waves)) return;
    if (p == 0 && e->dec_ring && K <= 1280 && sl.total_rows <= 160 && launch_dec_ring(a, w, ldw, rows, N, K, ep, ws, wsb, 0, st))
      return;
    launch_gemm(a, w, ldw, rows, N, K, ep, ws, wsb, st);
  };
  // residual-producing GEMMs also apply the LayerNorm that consumes the residual (EPI_RESID_LN: fused into
  // the split-K combine on the skinny path): out -> ln2, cout -> ln3, fc2 -> next layer's ln1
  auto resid_ln = [&](const float* g, const float* b, const float* bias) {
    GemmEpi ep = epi_of(EPI_RESID_LN, x, d, bias);
    ep.ln_g = g; ep.ln_b = b; ep.ln_out = hb; ep.ln_ld = d;
    return ep;
  };
  // <= 16 rows: the LayerNorms after out and cout run inside their consumers (cq, fc1), from the residual and
  // the per-(16-column tile, row) sums their producers write (two combine launches fewer per layer)
  const bool ln_fuse = sl.total_rows <= 16 && e->dec_gemv && e->dec_gemv_ln && gemv_ln_fusable(rows, d, d, d);
  float* lnstat = nullptr;
  if (ln_fuse) {
    e->d_lnstat.ensure(2 * 128 * 16 * 2 * 4);
    lnstat = e->d_lnstat.as<float>() + (r0 == 0 ? 0 : 128 * 16 * 2);
  }
  auto resid_stat = [&](const float* bias) {
    GemmEpi ep = epi_of(EPI_RESID_F32, x, d, bias);
    ep.stat_out = lnstat;
    return ep;
  };
  auto ln_operand = [&](const float* g, const float* b) {
    GemmA a = amat(nullptr, d);
    a.lnx = x; a.ln_g = g; a.ln_b = b; a.ln_stat = lnstat; a.ln_tiles = d / 16;
    return a;
  };
  // fc2 -> the next layer's ln1 the same way: fc2 (K = 4d) writes the residual and its statistics without split-K,
  // the next layer's qkv normalises its operand (the same for every layer of a pass, so layer l > 0's qkv knows)
  const bool fc2_fuse = ln_fuse && e->dec_gemv_ln_fc2 && gemv_ln_fusable(rows, d, 4 * d, d);
  bf16* kc = skv + (size_t)(2 * l) * skv_layer;
  bf16* vc = skv + (size_t)(2 * l + 1) * skv_layer;
  {
    GemmEpi ep = epi_of(EPI_DEC_QKV, q, d, W.qkv_b);
    ep.kcache = kc; ep.vcache = vc; ep.row_hyp = row_hyp; ep.row_pos = row_pos;
    ep.d = d; ep.n_head = H; ep.head_dim = 64; ep.n_ctx = C;
    gemm(DEC_QKV, (fc2_fuse && l > 0) ? ln_operand(W.ln1_w, W.ln1_b) : amat(hb, d), W.qkv_w, d, 3 * d, d, ep);
  }
  {
    ProfScope ps(e, P_SELF_ATTN, st, 0, 0, true);
    launch_self_attn(q, d, kc, vc, lin, row_hyp, row_pos, done, ao, d, rows, H, C, e->dstat(P_SELF_ATTN), st, ps.a, ps.b,
                     sl.total_rows, cross_group);
  }
  gemm(DEC_OUT, amat(ao, d), W.out_w, d, d, d,
       ln_fuse ? resid_stat(W.out_b) : resid_ln(W.ln2_w, W.ln2_b, W.out_b));
  // cq: when the skinny split-K path runs it and no attention is captured, its slabs stay in the scratch and
  // the cross-attention kernel sums them while loading q (no combine launch)
  CrossFuse fz;
  {
    GemmEpi ep = epi_of(EPI_BF16, q, d, W.cq_b);
    const int pcq = plan_of(DEC_CQ);
    const int gsk = (sl.total_rows <= 32 && e->dec_gemv) ? gemv_splits(rows, d, d, nullptr) : 0;
    const int sk = gsk > 0 ? gsk
                 : pcq == -1 ? skinny_splits(rows, d, d, wsb)
                             : (pcq > 0 && e->dec_kr[DEC_CQ] > 0 ? (d + e->dec_kr[DEC_CQ] - 1) / e->dec_kr[DEC_CQ] : 1);
    if ((e->cross_fuse & 1) && !(attn && align_map) && sk > 1) {
      ep.defer_combine = 1;
      fz.q_part = ws; fz.q_splits = sk; fz.q_rows = rows; fz.q_bias = W.cq_b;
    }
    gemm(DEC_CQ, ln_fuse ? ln_operand(W.ln2_w, W.ln2_b) : amat(hb, d), W.cq_w, d, d, d, ep);
  }
  if ((e->cross_fuse & 2) && e->cross_mode == 0) fz.cnt = e->d_cross_cnt.as<int>() + (size_t)r0 * H;
  fz.tf = (attn && align_map && e->cross_tf) ? 1 : 0;
  fz.mfma = e->cross_mfma;
  if (e->cross_mfma_fuse && e->cross_mode == 0) fz.tf_cnt = e->d_cross_cnt.as<int>() + (size_t)r0 * H;
  float* probs = nullptr;
  const int* hmap = nullptr;
  if (attn && align_map) {
    const auto& mp = (*align_map)[l];
    bool any = false;
    for (int v : mp) any |= v >= 0;
    if (any) {
      HIP_OK(hipMemcpyAsync(e->d_head_map.p, mp.data(), H * 4, hipMemcpyHostToDevice, st));
      probs = attn + (size_t)r0 * n_align * T;
      hmap = e->d_head_map.as<int>();
    }
  }
  if (mid) HIP_OK(hipEventRecord(mid, st));
  if (e->cross_mode == 1 && e->tf_nwin > 0 && attn && align_map) {
    // factored form, alignment pass: this layer's K/V panels of the pass's windows projected on MFMA (the wm_cross_kv
    // GEMM restricted to one layer: 2 x d x d x T flops per window), then the projected form's teacher-forced kernel
    // over them (window = hypothesis index of the pass).  ~2.5x fewer flops than the factored attention at ~100
    // rows per window, and all of it on the matrix cores.
    const int nw = e->tf_nwin;
    GemmEpi ep = epi_of(EPI_CROSS_KV, e->a_kv.p, 0, e->Wf("dec.ckv.b") + (size_t)l * 2 * d);
    ep.rpb = T; ep.d = d; ep.head_dim = 64; ep.n_head = H; ep.n_slots = nw; ep.slot0 = 0;
    gemm_p(e, P_CROSSKV_GEMM, amat(e->a_enc.as<bf16>(), d), e->Wb("dec.ckv.w") + (size_t)l * 2 * d * d, d, nw * T, 2 * d, d,
           ep, st);
    const bf16* kv = e->a_kv.as<bf16>();
    const size_t po = (size_t)r0 * H * 16;
    ProfScope ps(e, P_CROSS_ATTN, st, 0, 0, true);
    launch_cross_attn(q, d, kv, kv + (size_t)nw * H * T * 64, T, nullptr, row_hyp, done, ao, d, rows, H, cross_group,
                      e->s_pm.as<float>() + po, e->s_pl.as<float>() + po, e->s_po.as<float>() + po * 64, probs, hmap,
                      n_align, sl.total_rows, e->cross_cap, fz, e->dstat(P_CROSS_ATTN), st, ps.a, ps.b);
  } else if (e->cross_mode == 1) {
    // factored: q' = Wk_h^T q_h, attention over the encoder output, split merge + Wv_h (attn_xenc.hip)
    const int splits = xattn_splits(sl.total_rows, cross_group, H, T, d);
    const size_t prow = (size_t)H * d;
    bf16* qp = e->s_qp.as<bf16>() + (size_t)r0 * prow;
    bf16* pu = e->s_pu.as<bf16>() + (size_t)r0 * 16;         // blocked layout: rows are 16-element records
    float* pml = e->s_pml.as<float>() + (size_t)r0 * H * 2;
    const bf16* wkt = e->xwkt.as<bf16>() + (size_t)l * H * d * 64;
    const bf16* wv = e->xwvb.as<bf16>() + (size_t)l * H * d * 64;
    const float* bv = e->Wf("dec.ckv.b") + (size_t)l * 2 * d + d;
    {
      ProfScope ps(e, P_DEC_GEMM, st, 2.0 * rows * H * d * 64, 2.0 * H * d * 64 + 2.0 * rows * d + 2.0 * rows * prow);
      launch_xq(q, d, fz, wkt, qp, rows, H, d, st);
    }
    {
      ProfScope ps(e, P_CROSS_ATTN, st, 0, 0, true);
      launch_xattn(qp, e->xenc.p, e->cross_fp8 ? e->xscale.as<float>() : nullptr, e->d_hyp_slot.as<int>(), row_hyp, done, rows, sl.total_rows, cross_group, H, T,
                   d, splits, e->xsnake ? (l & 1) : 0, e->xkeep, pu, pml, probs, hmap, n_align, e->dstat(P_CROSS_ATTN), st, ps.a, ps.b);
    }
    {
      ProfScope ps(e, P_CROSS_COMB, st, 2.0 * rows * d * d, 2.0 * d * d + 2.0 * splits * rows * prow + 2.0 * rows * d);
      launch_xcomb_vo(pu, pml, splits, sl.total_rows, wv, bv, row_hyp, done, ao, d, rows, H, d, T, probs, hmap, n_align, st);
    }
  } else if (e->cross_kv_fp8 == 1) {
    // projected form, fp8 panels: same launcher rules on the F8 kernel instantiations
    const size_t po = (size_t)r0 * H * 16;
    const unsigned char* c8 = e->ckv.as<unsigned char>();
    const unsigned char* x8 = e->ckv_exp.as<unsigned char>();
    CrossKv8 kv;
    kv.k = c8 + (size_t)(2 * l) * ckv_layer;
    kv.v = c8 + (size_t)(2 * l + 1) * ckv_layer;
    kv.kexp = x8 + (size_t)(2 * l) * cexp_layer;
    kv.vexp = x8 + (size_t)(2 * l + 1) * cexp_layer;
    ProfScope ps(e, P_CROSS_ATTN, st, 0, 0, true);
    launch_cross_attn_fp8(q, d, kv, T, e->d_hyp_slot.as<int>(), row_hyp, done, ao, d, rows, H, cross_group,
                          e->s_pm.as<float>() + po, e->s_pl.as<float>() + po, e->s_po.as<float>() + po * 64, probs, hmap,
                          n_align, sl.total_rows, e->cross_cap, fz, e->dstat(P_CROSS_ATTN), st, ps.a, ps.b);
  } else {
    const size_t po = (size_t)r0 * H * 16;
    ProfScope ps(e, P_CROSS_ATTN, st, 0, 0, true);
    launch_cross_attn(q, d, ckv + (size_t)(2 * l) * ckv_layer, ckv + (size_t)(2 * l + 1) * ckv_layer, T,
                      e->d_hyp_slot.as<int>(), row_hyp, done, ao, d, rows, H, cross_group, e->s_pm.as<float>() + po,
                      e->s_pl.as<float>() + po, e->s_po.as<float>() + po * 64, probs, hmap, n_align, sl.total_rows,
                      e->cross_cap, fz, e->dstat(P_CROSS_ATTN), st, ps.a, ps.b);
  }
  if (probs) HIP_OK(hipStreamSynchronize(st));   // the head map buffer is reused by the next layer
  gemm(DEC_COUT, amat(ao, d), W.cout_w, d, d, d,
       ln_fuse ? resid_stat(W.cout_b) : resid_ln(W.ln3_w, W.ln3_b, W.cout_b));
  {
    GemmEpi ep = epi_of(EPI_BF16, ff, 4LL * d, W.fc1_b);
    ep.act = 1;
    gemm(DEC_FC1, ln_fuse ? ln_operand(W.ln3_w, W.ln3_b) : amat(hb, d), W.fc1_w, d, 4 * d, d, ep);
  }
  if (l + 1 < L) {
    const auto& Wn = dec_weights(e)[l + 1];
    gemm(DEC_FC2, amat(ff, 4LL * d), W.fc2_w, 4LL * d, d, 4 * d,
         fc2_fuse ? resid_stat(W.fc2_b) : resid_ln(Wn.ln1_w, Wn.ln1_b, W.fc2_b));
  } else {
    gemm(DEC_FC2, amat(ff, 4LL * d), W.fc2_w, 4LL * d, d, 4 * d, epi_of(EPI_RESID_F32, x, d, W.fc2_b));
  }
}

// One decoder pass over `rows` rows; logits for the n_logit rows listed in logit_rows (device; nullptr =
// rows 0..n_logit-1) go to `logits`.  Optional cross-attention capture (align): head_map per layer computed
// by caller.
//
// Decode steps (logit_rows == nullptr, n_logit == rows, no capture) with enough rows split the rows into two
// slices on two streams, the second started when the first reaches its layer-0 cross-attention.  Each
// slice then alternates a latency-bound chain of skinny weight GEMMs with an HBM-bound cross-attention,
// and the two slices run in opposite phase: one slice's GEMM chain executes while the other streams its
// cross-KV, so the step costs ~max(chain, cross) per layer instead of their sum.  The weights are read once
// per slice (46 MB per layer for large-v3, against 1.15 GB of cross-KV), and every row sees exactly the
// same arithmetic as in a one-slice pass.
void decoder_pass(wm_engine* e, int rows, const int* row_tok, const int* row_pos, const int* row_hyp, const int* done,
                  const int* lin, const int* logit_rows, int n_logit, float* logits,
                  const std::vector<std::vector<int>>* align_map, int n_align, float* attn, int cross_group,
                  hipStream_t st, int* err = nullptr) {
  const auto& m = e->dm;
  const int d = m.n_state, L = m.n_dec_layer;
  const auto& W0 = dec_weights(e)[0];
  // host-side check of the row buffers against what the launches below index (rows of the pass, and the
  // final LayerNorm's gathered logit rows)
  if ((size_t)rows * d * 4 > e->s_x.bytes || (size_t)std::max(rows, n_logit) * d * 2 > e->s_hb.bytes)
    throw std::runtime_error("decoder_pass: row buffers smaller than the pass (" + std::to_string(rows) + " rows, " +
                             std::to_string(n_logit) + " logit rows)");
  if (e->cross_mode == 1) {
    // factored cross-attention scratch for the whole pass (slices index it by absolute row), and the
    // per-head Wk^T layout (packed once per upload of dec.ckv.w)
    const int H = m.n_head, T = m.n_audio_ctx;
    const size_t prow = (size_t)H * d;
    const int splits = xattn_splits(rows, cross_group, H, T, d);
    e->s_qp.ensure((size_t)rows * prow * 2);
    e->s_pu.ensure((size_t)splits * rows * prow * 2);
    e->s_pml.ensure((size_t)splits * rows * H * 2 * 4);
    if (!e->xwkt_ready) {
      e->xwkt.ensure((size_t)L * H * d * 64 * 2);
      e->xwvb.ensure((size_t)L * H * d * 64 * 2);
      launch_xpack(e->Wb("dec.ckv.w"), e->xwkt.as<bf16>(), e->xwvb.as<bf16>(), L, H, d, st);
      e->xwkt_ready = true;
    }
    if (!e->xenc.p) throw std::runtime_error("decoder: no encoder slots (wm_reserve + wm_cross_kv first)");
  }
  int h0 = (rows / 2 / cross_group) * cross_group;
  const bool split = e->dec_split && logit_rows == nullptr && n_logit == rows && attn == nullptr && h0 >= 16 &&
                     rows - h0 >= 16;
  std::vector<DecSlice> sl;
  if (split) {
    if (!e->st2) {
      int lo = 0, hi = 0;
      HIP_OK(hipDeviceGetStreamPriorityRange(&lo, &hi));
      HIP_OK(hipStreamCreateWithPriority(&e->st2, hipStreamNonBlocking, hi));
      HIP_OK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&e->ev_mid, hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    }
    sl.push_back({0, h0, rows, st, &e->gemm_ws});
    sl.push_back({h0, rows - h0, rows, e->st2, &e->gemm_ws2});
    HIP_OK(hipEventRecord(e->ev_fork, st));
    HIP_OK(hipStreamWaitEvent(e->st2, e->ev_fork, 0));
  } else {
    sl.push_back({0, rows, rows, st, &e->gemm_ws});
  }
  for (const auto& s : sl) {
    ProfScope ps(e, P_DEC_OTHER, s.st);
    float* x = e->s_x.as<float>() + (size_t)s.r0 * d;
    launch_embed(row_tok + s.r0, row_pos + s.r0, e->Wb("dec.embed"), e->Wf("dec.pos"), x, s.rows, d, m.n_vocab, m.n_text_ctx,
                 s.st, err);
    launch_layernorm(x, d, nullptr, s.rows, d, W0.ln1_w, W0.ln1_b, e->s_hb.as<bf16>() + (size_t)s.r0 * d, d, s.st);
  }
  for (int l = 0; l < L; ++l) {
    for (size_t i = 0; i < sl.size(); ++i) {
      if (split && l == 0 && i == 1) HIP_OK(hipStreamWaitEvent(e->st2, e->ev_mid, 0));
      decoder_layer(e, sl[i], l, row_pos, row_hyp, done, lin, align_map, n_align, attn, cross_group,
                    (split && l == 0 && i == 0) ? e->ev_mid : nullptr);
    }
  }
  // logits == nullptr (wm_language_id): the pass stops here, the rows' last hidden states (before dec.ln) stay in s_x
  for (const auto& s : sl) {
    if (!logits) break;
    const int nl = split ? s.rows : n_logit;
    const int* lr = split ? nullptr : logit_rows;
    {
      ProfScope ps(e, P_DEC_OTHER, s.st);
      launch_layernorm(e->s_x.as<float>() + (size_t)s.r0 * d, d, lr, nl, d, e->Wf("dec.ln.w"), e->Wf("dec.ln.b"),
                       e->s_hb.as<bf16>() + (size_t)s.r0 * d, d, s.st);
    }
    const size_t wsb = 64ull << 20;
    s.ws->ensure(wsb);
    ProfScope ps(e, P_LOGITS_GEMM, s.st, 2.0 * nl * m.n_vocab * d, gemm_bytes(nl, m.n_vocab, d, 4));
    launch_gemm(amat(e->s_hb.as<bf16>() + (size_t)s.r0 * d, d), e->Wb("dec.embed"), d, nl, m.n_vocab, d,
                epi_of(EPI_F32, logits + (size_t)s.r0 * m.n_vocab, m.n_vocab, nullptr), s.ws->as<float>(), wsb, s.st);
  }
  if (split) {
    HIP_OK(hipEventRecord(e->ev_join, e->st2));
    HIP_OK(hipStreamWaitEvent(st, e->ev_join, 0));
  }
}

void check_weights(wm_engine* e) {
  for (auto& kv : e->slots)
    if (!kv.second.set) throw std::runtime_error("weight not set: " + kv.first);
}

void reserve(wm_engine* e, int n_slots, int n_hyp) {
  const auto& m = e->dm;
  const int H = m.n_head, C = m.n_text_ctx, T = m.n_audio_ctx, L = m.n_dec_layer;
  if (n_slots > e->n_slots) {
    // factored mode keeps each window's encoder output (T x d bf16); projected mode its L x 2 K/V panels
    e->ckv.release();
    e->ckv_exp.release();
    e->kv8_stage.release();
    e->xenc.release();
    e->xscale.release();
    if (e->cross_mode == 1) {
      // bf16: tile-blocked slots (attn_xenc.hip xblock_kernel), T padded to whole 32-row tiles
      e->xenc.ensure(e->cross_fp8 ? (size_t)n_slots * T * m.n_state : (size_t)n_slots * xblock_slot_elems(T, m.n_state) * 2);
      if (e->cross_fp8) e->xscale.ensure((size_t)n_slots * T * 4);
    } else if (e->cross_kv_fp8 == 1) {
      e->ckv.ensure((size_t)L * 2 * n_slots * H * T * 64);
      e->ckv_exp.ensure((size_t)L * 2 * n_slots * H * T);
    } else {
      e->ckv.ensure((size_t)L * 2 * n_slots * H * T * 64 * 2);
    }
    e->n_slots = n_slots;
  }
  if (n_hyp > e->n_hyp_cap) {
    e->skv.release();
    e->skv.ensure((size_t)L * 2 * n_hyp * H * C * 64 * 2);
    e->n_hyp_cap = n_hyp;
    const size_t nh = n_hyp;
    e->d_tokens.ensure(nh * C * 4);
    e->d_lin.ensure(nh * C * 4);
    e->d_seq_len.ensure(nh * 4);
    e->d_done.ensure(nh * 4);
    e->d_cum.ensure(nh * 4);
    e->d_row_tok.ensure(nh * 4);
    e->d_row_pos.ensure(nh * 4);
    e->d_row_hyp.ensure(nh * 4);
    e->d_hyp_slot.ensure(nh * 4);
    e->d_cand_tok.ensure(nh * 9 * 4);
    e->d_cand_lp.ensure(nh * 9 * 4);
    e->d_ns.ensure(nh * 4);
    e->d_fin_tok.ensure(nh * 16 * C * 4);
    e->d_fin_len.ensure(nh * 16 * 4);
    e->d_fin_cum.ensure(nh * 16 * 4);
    e->d_n_fin.ensure(nh * 4);
  }
  e->d_n_active.ensure(8 * 4);
  e->d_suppress.ensure((size_t)SEARCH_SB * 8);
  e->d_head_map.ensure((size_t)H * 4);
}

// The decode's device error word (d_n_active[1..3]) -> exception (wm_generate returns -1 with this text).
void check_decode_error(const int* w) {
  if (w[0] == 0) return;
  std::string what;
  if (w[0] == WM_ERR_TOKEN_RANGE)
    what = "decoder input token " + std::to_string(w[1]) + " at position " + std::to_string(w[2]) + " outside its table";
  else
    what = std::string(w[0] == WM_ERR_NONFINITE ? "non-finite (NaN / inf) logits" : "no token allowed by the logit rules") +
           " for hypothesis " + std::to_string(w[1]) + " after " + std::to_string(w[2]) + " generated tokens";
  throw std::runtime_error("generate: " + what + "; the decode was stopped");
}

// Search parameters shared by both decode loops (per-call fields: mode, tables, records)
SearchParams search_params(wm_engine* e, const wm_generate_args* a, float* logits, int P) {
  const auto& m = e->dm;
  SearchParams sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.logits = logits; sp.ldl = m.n_vocab; sp.V = m.n_vocab;
  sp.tokens = e->d_tokens.as<int>(); sp.n_ctx = m.n_text_ctx; sp.seq_len = e->d_seq_len.as<int>(); sp.sample_begin = P;
  sp.suppress_bits = e->d_suppress.as<unsigned long long>();
  static const int sel_abl = [] {
    const char* v = std::getenv("VLOG_AMD_SEL_ABL");
    return v ? std::atoi(v) : 0;
  }();
  sp.abl = sel_abl;
  sp.suppress_blank = a->suppress_blank; sp.blank = m.blank;
  sp.eot = m.eot; sp.no_timestamps = m.no_timestamps; sp.ts_begin = m.timestamp_begin;
  sp.max_initial = a->max_initial_timestamp_index; sp.with_ts = a->with_timestamps; sp.done = e->d_done.as<int>();
  sp.seed = a->seed; sp.max_length = a->max_length;
  sp.inv_temperature = a->temperature > 0.f ? 1.0f / a->temperature : 1.0f;
  sp.cum = e->d_cum.as<float>(); sp.row_tok = e->d_row_tok.as<int>(); sp.row_pos = e->d_row_pos.as<int>();
  sp.n_active = e->d_n_active.as<int>(); sp.cand_tok = e->d_cand_tok.as<int>(); sp.cand_lp = e->d_cand_lp.as<float>();
  sp.err = e->d_n_active.as<int>() + 1;
  // 0 in either field is "off" (a zero-filled ABI 2 struct); validated in generate.  The values are baked into a
  // captured step graph, which is safe: every StepGraph lives inside one wm_generate call and is never reused.
  sp.rep_penalty = a->repetition_penalty == 0.f ? 1.0f : a->repetition_penalty;
  sp.no_repeat_ngram = a->no_repeat_ngram_size;
  if (e->n_seq_bias > 0) {
    sp.bias_off = e->d_sb_off.as<int>(); sp.bias_tok = e->d_sb_tok.as<int>(); sp.bias_val = e->d_sb_val.as<float>();
    sp.n_bias = e->n_seq_bias;
  }
  return sp;
}

void upload_suppress(wm_engine* e, const wm_generate_args* a, hipStream_t st) {
  const int V = e->dm.n_vocab;
  std::vector<unsigned char> sup(V, 0);
  for (int i = 0; i < a->n_suppress; ++i)
    if (a->h_suppress[i] >= 0 && a->h_suppress[i] < V) sup[a->h_suppress[i]] = 1;
  std::vector<unsigned long long> supbits(SEARCH_SB);
  search_suppress_bits(sup.data(), V, supbits.data());
  HIP_OK(hipMemcpyAsync(e->d_suppress.p, supbits.data(), SEARCH_SB * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipStreamSynchronize(st));
}

// TEST ONLY (options debug_nan_row / debug_nan_count): NaN into logits rows before selection (bytes 0xFF are a NaN)
void debug_nan(wm_engine* e, float* logits, int rows, hipStream_t s) {
  if (e->dbg_nan_row >= 0 && e->dbg_nan_row < rows) {
    const int n = std::min(e->dbg_nan_count, rows - e->dbg_nan_row);
    HIP_OK(hipMemsetAsync(logits + (size_t)e->dbg_nan_row * e->dm.n_vocab, 0xFF, (size_t)n * e->dm.n_vocab * 4, s));
  }
}

// The decode steps of one decode loop (generate, generate_rows, generate_rows_beam): eager, or a captured graph's replay.
//
// A decode step's launches are identical from step to step: every per-step quantity (tokens, positions,
// lineage, done flags, sequence lengths) lives in device memory and is advanced by the select kernels, so
// after one eager step (which sizes every scratch buffer) the step is captured once as a HIP graph and
// replayed: one graph launch per step instead of ~11 kernel launches per layer.  Not with the event profiler
// (its events are per launch) or the two-stream split.  The loop issues everything (steps, event passes, polls) on
// `ds`: the replay stream, forked from `st` here and joined to it by finish(), or `st` itself without a graph.
// Steps that run eagerly: the first, the one after rows_changed(), and the one after a buffer moved.
struct StepGraph {
  wm_engine* e;
  hipStream_t st, ds;
  const bool use;
  int captures = 0;
  hipGraphExec_t exec = nullptr;
  bool capturing = false;
  bool eager_next = true;                   // the next step runs eagerly (sizes scratch), the one after is captured
  long long gen = -1;                       // realloc_gen() at capture
  StepGraph(wm_engine* e, hipStream_t st) : e(e), st(st), ds(st), use(e->dec_graph && !e->prof_on && !e->dec_split) {
    if (!use) return;
    if (!e->gst) {
      HIP_OK(hipStreamCreateWithFlags(&e->gst, hipStreamNonBlocking));
      HIP_OK(hipEventCreateWithFlags(&e->ev_g0, hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&e->ev_g1, hipEventDisableTiming));
    }
    HIP_OK(hipEventRecord(e->ev_g0, st));
    HIP_OK(hipStreamWaitEvent(e->gst, e->ev_g0, 0));
    ds = e->gst;
  }
  StepGraph(const StepGraph&) = delete;
  // An exception leaves the loop through here: the stream leaves capture mode before the error is reported
  ~StepGraph() {
    if (capturing) {
      hipGraph_t g = nullptr;
      if (hipStreamEndCapture(ds, &g) == hipSuccess && g) (void)hipGraphDestroy(g);
    }
    drop();
  }
  void drop() {
    if (exec) (void)hipGraphExecDestroy(exec);
    exec = nullptr;
  }
  // the pass's row count changed (compaction, an event pass): the captured graph no longer describes the step
  void rows_changed() {
    drop();
    eager_next = true;
  }
  // One decode step: launches(stream) issues it.
  template <class F> void step(F&& launches) {
    if (exec && gen != realloc_gen()) rows_changed();   // a buffer the graph points into moved: an eager step re-sizes
    if (!use || eager_next) {
      eager_next = false;
      launches(ds);
      return;
    }
    if (!exec) {
      ++captures;
      hipGraph_t g = nullptr;
      gen = realloc_gen();
      HIP_OK(hipStreamBeginCapture(ds, hipStreamCaptureModeThreadLocal));
      capturing = true;
      launches(ds);
      capturing = false;
      HIP_OK(hipStreamEndCapture(ds, &g));
      const hipError_t ie = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIP_OK(ie);
      if (gen != realloc_gen()) throw std::runtime_error("decode step graph: a buffer moved during capture");
    }
    HIP_OK(hipGraphLaunch(exec, ds));
  }
  // The loop is over: `st` waits for the replay stream, and the graph's last replay completes before it is destroyed.
  void finish() {
    if (use) {
      HIP_OK(hipEventRecord(e->ev_g1, ds));
      HIP_OK(hipStreamWaitEvent(st, e->ev_g1, 0));
    }
    if (exec) {
      HIP_OK(hipStreamSynchronize(ds));
      drop();
    }
  }
};

// The per-window view of a call's prompts (ABI 4): every window's prompt length, sot index and length limit, whether
// the caller passed them per window or as one value.  `ragged` is set when the caller passed any of h_prompt_lens /
// h_sot_indices / h_max_lengths, and means one thing: the selection kernels read the per-hypothesis device tables
// (without it a call launches exactly the one-length kernels, with null table pointers).
struct WinArgs {
  bool ragged = false;
  bool same_len = true;           // every window has the same prompt length (then the prefill keeps its grouping)
  bool any_sot = false;           // some window has a sot index (the passes then produce no-speech logit rows)
  int Pmax = 0;                   // the longest prompt (scratch sizing, pass limit)
  int max_gen = 0;                // the most tokens any window may generate: max over w of ml[w] - len[w]
  std::vector<int> len, sot, ml;  // [W]
};

// Validates the prompts of a call (nothing has been launched yet) and resolves the per-window values.
WinArgs window_args(wm_engine* e, const wm_generate_args* a) {
  const int C = e->dm.n_text_ctx, V = e->dm.n_vocab;
  const int W = a->n_windows, P = a->prompt_len;
  WinArgs wa;
  wa.ragged = a->h_prompt_lens || a->h_sot_indices || a->h_max_lengths;
  if (!wa.ragged) {
    if (P <= 0 || P >= a->max_length || a->max_length > C) throw std::runtime_error("generate: bad prompt_len/max_length");
    if (a->sot_index >= P) throw std::runtime_error("generate: sot_index outside the prompt");
    for (int i = 0; i < W * P; ++i)
      if (a->h_prompts[i] < 0 || a->h_prompts[i] >= V) throw std::runtime_error("generate: prompt token out of the vocabulary");
    wa.Pmax = P;
    wa.max_gen = a->max_length - P;
    wa.len.assign(W, P); wa.sot.assign(W, a->sot_index); wa.ml.assign(W, a->max_length);
    wa.any_sot = a->sot_index >= 0;
    return wa;
  }
  if (P <= 0) throw std::runtime_error("generate: bad prompt_len/max_length");
  wa.len.resize(W); wa.sot.resize(W); wa.ml.resize(W);
  for (int w = 0; w < W; ++w) {
    const std::string who = "generate: window " + std::to_string(w) + ": ";
    const int n = a->h_prompt_lens ? a->h_prompt_lens[w] : P;
    const int ml = a->h_max_lengths ? a->h_max_lengths[w] : a->max_length;
    const int sot = a->h_sot_indices ? a->h_sot_indices[w] : a->sot_index;
    if (n <= 0 || n > P)
      throw std::runtime_error(who + "prompt length " + std::to_string(n) + " outside [1, prompt_len = " + std::to_string(P) + "]");
    if (ml > C || ml > a->max_length)
      throw std::runtime_error(who + "max length " + std::to_string(ml) + " above n_text_ctx or max_length");
    if (n >= ml)
      throw std::runtime_error(who + "prompt length " + std::to_string(n) + " leaves no room below its max length " +
                               std::to_string(ml));
    if (sot >= n) throw std::runtime_error(who + "sot index " + std::to_string(sot) + " outside its prompt");
    for (int p = 0; p < n; ++p) {                 // the padding behind the prompt is neither validated nor read
      const int t = a->h_prompts[(size_t)w * P + p];
      if (t < 0 || t >= V)
        throw std::runtime_error(who + "prompt token " + std::to_string(t) + " at position " + std::to_string(p) +
                                 " out of the vocabulary");
    }
    wa.len[w] = n; wa.ml[w] = ml; wa.sot[w] = sot;
    wa.Pmax = std::max(wa.Pmax, n);
    wa.max_gen = std::max(wa.max_gen, ml - n);
    if (n != wa.len[0]) wa.same_len = false;
    wa.any_sot |= sot >= 0;
  }
  return wa;
}

// Uploads the per-window tables of a ragged row-set decode and points the selection at the per-hypothesis ones
// (n_hyp entries, filled by hyp_start / beam_start as slots take windows).
void upload_window_tables(wm_engine* e, const WinArgs& wa, int n_hyp, SearchParams* sp, BeamParams* bp, hipStream_t st) {
  const size_t W = wa.len.size();
  e->d_win_len.ensure(W * 4);
  e->d_win_maxlen.ensure(W * 4);
  e->d_hyp_begin.ensure((size_t)n_hyp * 4);
  e->d_hyp_maxlen.ensure((size_t)n_hyp * 4);
  HIP_OK(hipMemcpyAsync(e->d_win_len.p, wa.len.data(), W * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_win_maxlen.p, wa.ml.data(), W * 4, hipMemcpyHostToDevice, st));
  // slots that no window has taken yet are skipped by the selection (done), but keep their rows defined
  HIP_OK(hipMemsetAsync(e->d_hyp_begin.p, 0, (size_t)n_hyp * 4, st));
  HIP_OK(hipMemsetAsync(e->d_hyp_maxlen.p, 0, (size_t)n_hyp * 4, st));
  sp->hyp_begin = e->d_hyp_begin.as<int>(); sp->hyp_maxlen = e->d_hyp_maxlen.as<int>();
  if (bp) { bp->hyp_begin = sp->hyp_begin; bp->hyp_maxlen = sp->hyp_maxlen; }
}

// The beam selection's parameters beside `sp` (whose tables, record arrays and per-hypothesis length tables it shares)
BeamParams beam_params(wm_engine* e, const wm_generate_args* a, const SearchParams& sp, int max_cand) {
  BeamParams bp;
  std::memset(&bp, 0, sizeof(bp));
  bp.beam = a->beam_size; bp.max_cand = max_cand; bp.n_ctx = e->dm.n_text_ctx; bp.sample_begin = a->prompt_len;
  bp.max_length = a->max_length;
  bp.eot = e->dm.eot; bp.cand_tok = sp.cand_tok; bp.cand_lp = sp.cand_lp; bp.tokens = sp.tokens; bp.lin = e->d_lin.as<int>();
  bp.seq_len = sp.seq_len; bp.cum = sp.cum; bp.done = sp.done; bp.row_tok = sp.row_tok; bp.row_pos = sp.row_pos;
  bp.fin_tok = e->d_fin_tok.as<int>(); bp.fin_len = e->d_fin_len.as<int>(); bp.fin_cum = e->d_fin_cum.as<float>();
  bp.n_fin = e->d_n_fin.as<int>(); bp.n_active = sp.n_active;
  bp.hyp_begin = sp.hyp_begin; bp.hyp_maxlen = sp.hyp_maxlen;
  if (sp.tok_lp) {
    bp.tok_lp = sp.tok_lp;
    bp.fin_lp = e->d_fin_lp.as<float>();
  }
  return bp;
}

float length_norm(const wm_generate_args* a, float cum, int n) {
  return cum / std::pow((float)std::max(n, 1), a->length_penalty);
}

// Host copies of one window's finished list (entry i: tokens from the first generated one) or of its beam_size live
// beams (entry b: the whole sequence, prompt included); entries are n_text_ctx apart in tok / lp.  lp: optional records.
struct BeamView { const int* tok; const int* len; const float* cum; const float* lp; };
struct BeamBest { const int* tok = nullptr; int len = 0; float cum = 0.f, score = -INFINITY; const float* lp = nullptr; };

// The result of one window's beam search: the finished candidates (beam_select keeps n_fin within max_cand; clamped
// here all the same), then, openai finalize, unfinished beams by sum_logprob until beam_size are ranked; the best
// length-normalised score wins.  Pw: the window's own prompt length.
BeamBest beam_best(const wm_generate_args* a, int C, int max_cand, int Pw, const BeamView& fin, int n_fin,
                   const BeamView& beams) {
  const int K = a->beam_size;
  BeamBest best;
  int n = 0;
  auto offer = [&](const int* t, int len, float c, const float* r) {
    const float s = length_norm(a, c, len);
    if (s > best.score) { best.tok = t; best.len = len; best.cum = c; best.score = s; best.lp = r; }
    ++n;
  };
  for (int i = 0; i < std::min(n_fin, max_cand); ++i)
    offer(fin.tok + (size_t)i * C, fin.len[i], fin.cum[i], fin.lp ? fin.lp + (size_t)i * C : nullptr);
  std::vector<int> order;
  for (int b = 0; b < K; ++b)
    if (beams.cum[b] > -INFINITY) order.push_back(b);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return beams.cum[x] > beams.cum[y]; });
  for (int b : order) {
    if (n >= K) break;
    offer(beams.tok + (size_t)b * C + Pw, beams.len[b] - Pw, beams.cum[b], beams.lp ? beams.lp + (size_t)b * C + Pw : nullptr);
  }
  return best;
}

// One window's result into the caller's arrays.  tok / lp / lpo start at the first generated token.  ns: the window's
// no-speech probability (nullptr: the caller writes h_no_speech at its end).  Per-step records, when the call asks for
// them: one per generated token, plus the final <|endoftext|> when the window ended on it (not at its length limit);
// NaN where the decode form keeps no such record.
void write_window_result(const wm_generate_args* a, const WinArgs& wa, int w, const int* tok, int n, float cum, float score,
                         const float* ns, const float* lp, const float* lpo) {
  const int ML = a->max_length;
  if (n < 0 || n > ML) throw std::runtime_error("generate: window " + std::to_string(w) + " has no result");
  for (int i = 0; i < n; ++i) a->h_tokens[(size_t)w * ML + i] = tok[i];
  a->h_lengths[w] = n;
  a->h_scores[w] = score;
  if (a->h_cum_logprob) a->h_cum_logprob[w] = cum;
  if (a->h_no_speech && ns) a->h_no_speech[w] = wa.sot[w] >= 0 ? *ns : 0.f;
  if (a->h_token_logprobs) {
    const int nr = std::min(ML, n + (wa.len[w] + n < wa.ml[w] ? 1 : 0));
    for (int i = 0; i < nr; ++i) {
      a->h_token_logprobs[(size_t)w * ML + i] = lp ? lp[i] : NAN;
      if (a->h_token_logprobs_other) a->h_token_logprobs_other[(size_t)w * ML + i] = lpo ? lpo[i] : NAN;
    }
  }
}

void write_stats(const wm_generate_args* a, long long passes, long long row_steps, long long refills, int captures) {
  if (a->h_steps) a->h_steps[0] = (int)passes;
  if (a->h_stats) {
    a->h_stats[0] = passes;
    a->h_stats[1] = row_steps;
    a->h_stats[2] = refills;
    a->h_stats[3] = captures;
  }
}

// wm_generate_multilingual: entries (offset into `table`, auto index), two ints each -> the chosen language tokens into
// `table`, on `s`.  `ent` must stay alive until the stream has taken it.
void lang_assign(wm_engine* e, const std::vector<int>& ent, int* table, hipStream_t s) {
  const LangCall* lc = e->call_lang;
  if (!lc || ent.empty()) return;
  e->d_la_ent.ensure(ent.size() * 4);
  HIP_OK(hipMemcpyAsync(e->d_la_ent.p, ent.data(), ent.size() * 4, hipMemcpyHostToDevice, s));
  launch_lang_assign((int)ent.size() / 2, e->d_la_ent.as<int>(), lc->d_top, lc->lang_begin, lc->n_langs, table, s);
}

// ... the row-set forms' per-window prompt table (every window is identified before the call's first pass)
void lang_assign_windows(wm_engine* e, int W, int P, hipStream_t s, std::vector<int>* ent) {
  const LangCall* lc = e->call_lang;
  if (!lc) return;
  for (int w = 0; w < W; ++w)
    if (lc->pos[w] >= 0) { ent->push_back(w * P + lc->pos[w]); ent->push_back(lc->aidx[w]); }
  // (sized for any event's list, so no event moves it under a captured step graph: a start lists its language row,
  // and the beam form's padding copies of it, at most 8 rows)
  e->d_la_ent.ensure((size_t)W * 8 * 2 * 4);
  lang_assign(e, *ent, e->d_win_prompt.as<int>(), s);
}

// ... the lockstep form: every hypothesis' token row, and the prefill rows (set i's rows start at pf_at[i])
void lang_assign_lockstep(wm_engine* e, int NH, int per, int pf_per, int C, const std::vector<int>& pf_at, hipStream_t s,
                          std::vector<int>* ent_tok, std::vector<int>* ent_row) {
  const LangCall* lc = e->call_lang;
  if (!lc) return;
  for (int h = 0; h < NH; ++h) {
    const int w = h / per;
    if (lc->pos[w] < 0) continue;
    ent_tok->push_back(h * C + lc->pos[w]); ent_tok->push_back(lc->aidx[w]);
    if (h % pf_per == 0) { ent_row->push_back(pf_at[h / pf_per] + lc->pos[w]); ent_row->push_back(lc->aidx[w]); }
  }
  lang_assign(e, *ent_tok, e->d_tokens.as<int>(), s);
  lang_assign(e, *ent_row, e->d_prow_tok.as<int>(), s);
}

// The lists of one row-set event pass, carved from one int array: the host image e->h_ev (zero-filled here; it lives on
// the engine until the next poll synchronises the stream) and, at the same offsets, its device copy d_ev:
// ptok, ppos, phyp, psrc [np] | row set [nr] | logit rows [nr + nsot] | start slots (groups), windows [nst] | live count
struct EventLists {
  struct Ptrs { int *ptok, *ppos, *phyp, *psrc, *rh, *lr, *hs, *ws, *n_live; } h, d;
  size_t n;
  EventLists(wm_engine* e, int np, int nr, int nsot, int nst) : n((size_t)4 * np + 2 * nr + nsot + 2 * nst + 1) {
    auto carve = [&](int* b) {
      return Ptrs{b, b + np, b + 2 * np, b + 3 * np, b + 4 * np, b + 4 * np + nr, b + 4 * np + 2 * nr + nsot,
                  b + 4 * np + 2 * nr + nsot + nst, b + 4 * np + 2 * nr + nsot + 2 * nst};
    };
    e->h_ev.assign(n, 0);
    e->d_ev.ensure(n * 4);
    h = carve(e->h_ev.data());
    d = carve(e->d_ev.as<int>());
  }
  void upload(wm_engine* e, hipStream_t s) const {
    HIP_OK(hipMemcpyAsync(e->d_ev.p, e->h_ev.data(), n * 4, hipMemcpyHostToDevice, s));
  }
};

// What a row-set decode shares with its driver: the queue of windows, the current pass's rows, the counts for h_stats.
struct RowSet {
  int W = 0, next = 0;            // windows of the call; the next one to start
  int nrows = 0;                  // rows of the current row set (event() sets it)
  long long passes = 0, row_steps = 0, refills = 0;
};
struct RowSetRules {
  int check;                      // decode passes between host polls
  long long pass_limit;           // a generous bound against a stuck loop
  int refill_min;                 // free units that make a refill worth its eager pass
  int compact_8ths;               // compaction once the live units fall to this many eighths of the row set ...
  bool compact;                   // ... if the call asked for it
  int n_done;                     // hypothesis slots whose done flags a poll reads
};

// The row-set decode loop of generate_rows (unit: a row) and generate_rows_beam (unit: a group of beam_size rows).
// The caller has listed the first windows' starts; then, every `check` passes, a poll (counters, done flags) and:
//   ended(done, s)   marks the units whose window ended (beam: finalises them) -> {live units, units in the row set}
//   rebuild(refill)  lists the next row set, starting windows in free units (refill) or dropping them (compaction)
//                    -> windows started
//   event(s)         one event pass over those lists (sets rs.nrows)
//   step(s)          one decode step's launches
template <class Ended, class Rebuild, class Event, class Step>
void run_row_set(wm_engine* e, StepGraph& graph, RowSet& rs, const RowSetRules& r, Ended&& ended, Rebuild&& rebuild,
                 Event&& event, Step&& step) {
  std::vector<int> h_done(r.n_done);
  int h_cnt[4] = {0, 0, 0, 0};                  // live hypotheses, error word
  auto event_pass = [&] {
    event(graph.ds);
    ++rs.passes;
    rs.row_steps += rs.nrows;
  };
  event_pass();
  int k = 1;                                    // decode passes since the last host check
  for (;;) {
    if (k >= r.check) {
      k = 0;
      HIP_OK(hipMemcpyAsync(h_cnt, e->d_n_active.p, sizeof(h_cnt), hipMemcpyDeviceToHost, graph.ds));
      HIP_OK(hipMemcpyAsync(h_done.data(), e->d_done.p, (size_t)r.n_done * 4, hipMemcpyDeviceToHost, graph.ds));
      HIP_OK(hipStreamSynchronize(graph.ds));
      check_decode_error(h_cnt + 1);
      const std::pair<int, int> units = ended(h_done.data(), graph.ds);
      const int n_live = units.first, n_free = units.second - n_live;
      if (n_live == 0 && rs.next >= rs.W) break;
      const bool refill = rs.next < rs.W && (n_free >= r.refill_min || n_live == 0);
      const bool compact = rs.next >= rs.W && r.compact && n_live * 8 <= units.second * r.compact_8ths;
      if (refill || compact) {
        rs.refills += rebuild(refill);
        const int before = rs.nrows;
        event_pass();
        if (rs.nrows != before) graph.rows_changed();
        k = 1;
        continue;
      }
    }
    graph.step(step);
    ++rs.passes;
    rs.row_steps += rs.nrows;
    ++k;
    if (rs.passes > r.pass_limit) throw std::runtime_error("generate: decode did not terminate");
  }
}

void generate_rows(wm_engine* e, const wm_generate_args* a, const WinArgs& wa, hipStream_t st);
void generate_rows_beam(wm_engine* e, const wm_generate_args* a, const WinArgs& wa, hipStream_t st);

void generate(wm_engine* e, const wm_generate_args* a, hipStream_t st) {
  check_weights(e);
  const auto& m = e->dm;
  const int C = m.n_text_ctx, V = m.n_vocab;
  const int W = a->n_windows, P = a->prompt_len;
  if (W <= 0) return;
  const WinArgs wa = window_args(e, a);
  const bool rag = wa.ragged, any_sot = wa.any_sot;
  if (!(a->repetition_penalty >= 0.f) || std::isinf(a->repetition_penalty))
    throw std::runtime_error("generate: repetition_penalty must be a finite value > 0 (0 or 1: off)");
  if (a->no_repeat_ngram_size < 0 || a->no_repeat_ngram_size > a->max_length)
    throw std::runtime_error("generate: no_repeat_ngram_size must be in [0, max_length] (0: off)");
  const bool beam = a->beam_size > 1 && a->temperature <= 0.f;
  const bool sampling = a->temperature > 0.f;
  const int per = beam ? a->beam_size : (sampling ? std::max(1, a->num_hypotheses) : 1);
  const int NH = W * per;
  if (beam && a->beam_size > 8) throw std::runtime_error("generate: beam_size <= 8 supported");
  for (int w = 0; w < W; ++w)
    if (a->h_slots[w] < 0 || a->h_slots[w] >= e->n_slots) throw std::runtime_error("generate: slot out of range");
  if (a->max_rows < 0) throw std::runtime_error("generate: max_rows must be >= 0");
  if (per == 1 && !beam && ((a->max_rows > 0 && a->max_rows < W) || a->compact)) {
    generate_rows(e, a, wa, st);
    return;
  }
  if (beam && a->max_rows > 0 && a->max_rows < NH) {
    if (a->max_rows < per) throw std::runtime_error("generate: max_rows must hold one window's beam");
    generate_rows_beam(e, a, wa, st);
    return;
  }
  if (a->max_rows > 0 && a->max_rows < W) throw std::runtime_error("generate: max_rows needs greedy, beam search or num_hypotheses 1");
  reserve(e, e->n_slots, NH);
  const bool rec = a->h_token_logprobs != nullptr;
  const int max_cand = beam ? std::max(1, (int)std::lround(a->beam_size * a->patience)) : 0;
  if (max_cand > 16) throw std::runtime_error("generate: beam_size * patience must be <= 16");

  // ---- host-side init of the state tables
  std::vector<int> tokens((size_t)NH * C, 0), lin((size_t)NH * C, 0), seq_len(NH, P), zeros(NH, 0), hyp_slot(NH);
  std::vector<int> hyp_ml;                         // ragged: the per-hypothesis length limits (seq_len holds the prompt lengths)
  std::vector<float> cum(NH, 0.f);
  // Beam search: the hypotheses of a window share its prompt, so the prompt is prefilled once per window (into
  // the first hypothesis' self-KV rows) and every hypothesis' lineage points its prompt positions there (the
  // lineage is what beam reordering copies; the cache itself is never copied).  Greedy / sampling keep one
  // prefill per hypothesis: their self-attention reads each row's own cache (no lineage table).
  for (int h = 0; h < NH; ++h) {
    const int w = h / per;
    hyp_slot[h] = a->h_slots[w];
    const int Pw = wa.len[w];
    seq_len[h] = Pw;
    for (int p = 0; p < Pw; ++p) tokens[(size_t)h * C + p] = a->h_prompts[(size_t)w * P + p];
    for (int p = 0; p < C; ++p) lin[(size_t)h * C + p] = (beam && p < Pw) ? w * per : h;
    if (beam && (h % per) != 0) cum[h] = -INFINITY;
  }
  if (rag) {
    // the selection's per-hypothesis tables: a lockstep decode fills them once, here
    hyp_ml.resize(NH);
    for (int h = 0; h < NH; ++h) hyp_ml[h] = wa.ml[h / per];
    e->d_hyp_begin.ensure((size_t)NH * 4);
    e->d_hyp_maxlen.ensure((size_t)NH * 4);
    HIP_OK(hipMemcpyAsync(e->d_hyp_begin.p, seq_len.data(), NH * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(e->d_hyp_maxlen.p, hyp_ml.data(), NH * 4, hipMemcpyHostToDevice, st));
  }
  // per-window seeds (wm_generate_seeded): hypothesis h = w * per + j draws as (seed of w, j); filled once, here
  const bool seeded = sampling && e->call_seeds != nullptr;
  std::vector<unsigned long long> hyp_seed;
  std::vector<int> hyp_key;
  if (seeded) {
    hyp_seed.resize(NH); hyp_key.resize(NH);
    for (int h = 0; h < NH; ++h) { hyp_seed[h] = e->call_seeds[h / per]; hyp_key[h] = h % per; }
    e->d_hyp_seed.ensure((size_t)NH * 8);
    e->d_hyp_key.ensure((size_t)NH * 4);
    HIP_OK(hipMemcpyAsync(e->d_hyp_seed.p, hyp_seed.data(), (size_t)NH * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(e->d_hyp_key.p, hyp_key.data(), (size_t)NH * 4, hipMemcpyHostToDevice, st));
  }
  HIP_OK(hipMemcpyAsync(e->d_tokens.p, tokens.data(), tokens.size() * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_lin.p, lin.data(), lin.size() * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_seq_len.p, seq_len.data(), NH * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_done.p, zeros.data(), NH * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_n_fin.p, zeros.data(), NH * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_cum.p, cum.data(), NH * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_hyp_slot.p, hyp_slot.data(), NH * 4, hipMemcpyHostToDevice, st));
  upload_suppress(e, a, st);
  const int counter0[4] = {NH, 0, 0, 0};          // live hypotheses; error word cleared
  HIP_OK(hipMemcpyAsync(e->d_n_active.p, counter0, sizeof(counter0), hipMemcpyHostToDevice, st));
  if (rec) {
    e->d_tok_lp.ensure((size_t)NH * C * 4);
    if (!beam) e->d_tok_lp_o.ensure((size_t)NH * C * 4);
    else e->d_fin_lp.ensure((size_t)W * max_cand * C * 4);
  }

  // ---- prefill: rows (h, p) for every prompt position of every prefilled hypothesis (beam: one per window)
  const int pf_per = beam ? per : 1;                 // hypotheses per prefilled row set
  const int n_pf = NH / pf_per;
  // Ragged prompts: the prefilled sets are ordered by CLASS, and each class is one decoder pass over its own rows.
  // A class is a set of windows whose prompt rows form groups of one size g = (per / pf_per) * length, which is what
  // the cross-attention form follows (launch_cross_attn: 2..32 rows of one window take the matrix-core kernel in the
  // projected form, whose numerics differ from the f32 kernel's at bf16 rounding).  Windows whose g is at most 32
  // keep exactly the grouping, and so the kernel, of a call of their own; all longer prompts share one pass with
  // ungrouped rows (cross_group 1: the f32 kernels either way).  One length: one class, the pass as it always was.
  const int gmul = per / pf_per;
  std::vector<int> pf_cls(n_pf, 0), pf_order(n_pf);
  for (int i = 0; i < n_pf; ++i) {
    pf_order[i] = i;
    const int g = gmul * wa.len[i * pf_per / per];
    pf_cls[i] = (!rag || wa.same_len) ? g : (g <= 32 ? g : 0);
  }
  std::stable_sort(pf_order.begin(), pf_order.end(), [&](int x, int y) { return pf_cls[x] < pf_cls[y]; });
  std::vector<int> pf_off(n_pf + 1, 0), pf_at(n_pf);       // set i's rows start at pf_at[i]
  for (int k = 0; k < n_pf; ++k) {
    const int i = pf_order[k];
    pf_at[i] = pf_off[k];
    pf_off[k + 1] = pf_off[k] + wa.len[i * pf_per / per];
  }
  const int rows = pf_off[n_pf];
  const int nlog = any_sot ? 2 * NH : NH;
  const bool one_class = pf_cls[pf_order[0]] == pf_cls[pf_order[n_pf - 1]];
  // the pass's final LayerNorm gathers its nlog logit rows into s_hb rows [0, nlog): with the beam's shared
  // prefill (rows = W * P) that can exceed the pass rows, so the row buffers hold max(rows, NH, nlog)
  // (several classes: each pass writes its logit rows behind the nlog rows the selection reads, then they are moved)
  ensure_step(e, std::max(std::max(rows, NH), nlog), (one_class ? 1 : 2) * std::max(nlog, NH));
  std::vector<int> lr(nlog);
  {
    std::vector<int> rt(rows), rp(rows), rh(rows);
    for (int i = 0; i < n_pf; ++i)
      for (int p = 0; p < wa.len[i * pf_per / per]; ++p) {
        const int r = pf_at[i] + p, h = i * pf_per;
        rt[r] = tokens[(size_t)h * C + p]; rp[r] = p; rh[r] = h;
      }
    for (int h = 0; h < NH; ++h) {            // a hypothesis' logits come from its row set's last prompt row
      const int i = h / pf_per;
      lr[h] = pf_at[i] + wa.len[h / per] - 1;
      // (a ragged call's window without a sot index reads a row of its own; its no-speech result is dropped below)
      if (any_sot) lr[NH + h] = pf_at[i] + std::max(0, wa.sot[h / per]);
    }
    HIP_OK(hipMemcpyAsync(e->d_prow_tok.p, rt.data(), rows * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(e->d_prow_pos.p, rp.data(), rows * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(e->d_prow_hyp.p, rh.data(), rows * 4, hipMemcpyHostToDevice, st));
    if (one_class) HIP_OK(hipMemcpyAsync(e->d_logit_rows.p, lr.data(), nlog * 4, hipMemcpyHostToDevice, st));
    std::vector<int> ident(NH);
    for (int h = 0; h < NH; ++h) ident[h] = h;
    HIP_OK(hipMemcpyAsync(e->d_row_hyp.p, ident.data(), NH * 4, hipMemcpyHostToDevice, st));
    // multilingual call: the chosen language tokens into every hypothesis' prompt and into the prefill rows
    std::vector<int> ent_tok, ent_row;
    lang_assign_lockstep(e, NH, per, pf_per, C, pf_at, st, &ent_tok, &ent_row);
    HIP_OK(hipStreamSynchronize(st));   // host vectors above go out of scope
  }
  float* logits = e->s_logits.as<float>();
  int* err = e->d_n_active.as<int>() + 1;
  if (one_class) {
    decoder_pass(e, rows, e->d_prow_tok.as<int>(), e->d_prow_pos.as<int>(), e->d_prow_hyp.as<int>(), nullptr,
                 e->d_lin.as<int>(), e->d_logit_rows.as<int>(), nlog, logits, nullptr, 0, nullptr,
                 std::max(1, pf_cls[0]), st, err);
  } else {
    // every class' logit rows (relative to its first pass row) and the rows the selection expects them at, uploaded
    // once: [src rows of all classes | destination rows of all classes], nlog entries each
    float* tmp = logits + (size_t)nlog * V;
    struct Cls { int r0, nr, at, nc, group; };
    std::vector<Cls> classes;
    std::vector<int> tab(2 * (size_t)nlog);
    int at = 0;
    for (int k0 = 0; k0 < n_pf;) {
      const int cls = pf_cls[pf_order[k0]];
      int k1 = k0;
      while (k1 < n_pf && pf_cls[pf_order[k1]] == cls) ++k1;
      const int r0 = pf_off[k0], first = at;
      for (int k = k0; k < k1; ++k)
        for (int b = 0; b < pf_per; ++b) {
          const int h = pf_order[k] * pf_per + b;
          tab[at] = lr[h] - r0; tab[nlog + at] = h; ++at;
          if (any_sot) { tab[at] = lr[NH + h] - r0; tab[nlog + at] = NH + h; ++at; }
        }
      classes.push_back({r0, pf_off[k1] - r0, first, at - first, cls > 0 ? cls : 1});
      k0 = k1;
    }
    e->d_logit_rows.ensure(tab.size() * 4);
    HIP_OK(hipMemcpyAsync(e->d_logit_rows.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));         // (tab goes out of scope; the only host wait of the prefill)
    const int* dtab = e->d_logit_rows.as<int>();
    for (const Cls& c : classes) {
      decoder_pass(e, c.nr, e->d_prow_tok.as<int>() + c.r0, e->d_prow_pos.as<int>() + c.r0, e->d_prow_hyp.as<int>() + c.r0,
                   nullptr, e->d_lin.as<int>(), dtab + c.at, c.nc, tmp, nullptr, 0, nullptr, c.group, st, err);
      launch_rows_scatter(tmp, logits, dtab + nlog + c.at, c.nc, V, st);     // one launch moves the class' logit rows
    }
  }
  if (any_sot) launch_no_speech(logits + (size_t)NH * V, V, V, NH, m.no_speech, e->d_ns.as<float>(), st);

  SearchParams sp = search_params(e, a, logits, P);
  sp.mode = beam ? 1 : (sampling ? 2 : 0); sp.topk = beam ? a->beam_size + 1 : 1;
  if (rag) { sp.hyp_begin = e->d_hyp_begin.as<int>(); sp.hyp_maxlen = e->d_hyp_maxlen.as<int>(); }
  if (seeded) { sp.hyp_seed = e->d_hyp_seed.as<unsigned long long>(); sp.hyp_key = e->d_hyp_key.as<int>(); }
  if (rec) {
    sp.tok_lp = e->d_tok_lp.as<float>();
    if (!beam) sp.tok_lp_other = e->d_tok_lp_o.as<float>();
  }
  const BeamParams bp = beam_params(e, a, sp, max_cand);

  auto select = [&](int step) {
    sp.step = step;
    debug_nan(e, logits, NH, st);
    ProfScope ps(e, P_SELECT, st);
    launch_logits_select(sp, NH, st);
    if (beam) launch_beam_select(bp, W, st);
  };
  select(0);
  int steps = 1;
  long long row_steps = NH;                      // the prefill pass selects every hypothesis' first token
  const int max_steps = wa.max_gen;             // generated tokens (incl. the final one) <= max_length - P, per window
  const int check = std::max(1, a->check_every);
  StepGraph graph(e, st);
  const hipStream_t ds = graph.ds;
  // Beam compaction (a->compact): once the live windows' hypotheses fill <= 7/8 of the pass, the pass keeps only
  // them (row r -> hypothesis row_hyp[r], window groups stay contiguous); the beam state stays where it is, per
  // hypothesis (KV cache, lineage, tokens), so the rows' tokens / positions are gathered per pass (rows_fill) and
  // the selection reads its logits row by row.  Finished windows then stop costing GEMM rows in the tail.
  int nrows = NH;
  const bool bcompact = beam && a->compact;
  std::vector<int> h_rows(NH), h_bdone;
  for (int h = 0; h < NH; ++h) h_rows[h] = h;
  auto step_eager = [&](int step, hipStream_t s) {
    // logits rows of a decode step are the hypotheses themselves
    // greedy / sampling never reorder hypotheses: the lineage table is the identity and self-attention
    // reads each row's own cache directly (no dependent lineage load per key block)
    if (nrows < NH) {
      launch_rows_fill(nrows, e->d_row_hyp.as<int>(), e->d_prow_tok.as<int>(), e->d_prow_pos.as<int>(),
                       e->d_row_tok.as<int>(), e->d_row_pos.as<int>(), s);
      decoder_pass(e, nrows, e->d_prow_tok.as<int>(), e->d_prow_pos.as<int>(), e->d_row_hyp.as<int>(), e->d_done.as<int>(),
                   e->d_lin.as<int>(), nullptr, nrows, logits, nullptr, 0, nullptr, per, s, err);
    } else {
      decoder_pass(e, NH, e->d_row_tok.as<int>(), e->d_row_pos.as<int>(), e->d_row_hyp.as<int>(), e->d_done.as<int>(),
                   beam ? e->d_lin.as<int>() : nullptr, nullptr, NH, logits, nullptr, 0, nullptr, per, s, err);
    }
    sp.step = step;
    debug_nan(e, logits, nrows, s);
    ProfScope ps(e, P_SELECT, s);
    launch_logits_select(sp, nrows, s);
    if (beam) launch_beam_select(bp, W, s);
  };
  int poll[4] = {0, 0, 0, 0};                   // live count + error word
  if (bcompact) h_bdone.resize(NH);
  for (int step = 1; step < max_steps; ++step) {
    if ((step - 1) % check == 0) {
      HIP_OK(hipMemcpyAsync(poll, e->d_n_active.p, sizeof(poll), hipMemcpyDeviceToHost, ds));
      if (bcompact) HIP_OK(hipMemcpyAsync(h_bdone.data(), e->d_done.p, (size_t)NH * 4, hipMemcpyDeviceToHost, ds));
      HIP_OK(hipStreamSynchronize(ds));
      check_decode_error(poll + 1);
      if (poll[0] <= 0) break;
      // (beam passes are GEMM-row-bound at hundreds of rows, unlike the latency-bound greedy passes: compact at 7/8)
      if (bcompact && poll[0] * 8 <= nrows * 7) {
        // a finished window's hypotheses are all done (beam_select); keep the live windows' groups in order
        int n = 0;
        for (int r = 0; r < nrows; r += per) {
          const int h0 = h_rows[r];
          if (h_bdone[h0]) continue;
          for (int b = 0; b < per; ++b) h_rows[n + b] = h0 + b;
          n += per;
        }
        if (n > 0 && n < nrows) {
          nrows = n;
          HIP_OK(hipMemcpyAsync(e->d_row_hyp.p, h_rows.data(), (size_t)nrows * 4, hipMemcpyHostToDevice, ds));
          HIP_OK(hipStreamSynchronize(ds));
          sp.row_hyp = e->d_row_hyp.as<int>();
          graph.rows_changed();
        }
      }
    }
    graph.step([&](hipStream_t s) { step_eager(step, s); });
    ++steps;
    row_steps += nrows;
  }
  graph.finish();

  // ---- results
  std::vector<int> out_tok((size_t)NH * C), out_len(NH);
  std::vector<float> out_cum(NH), ns(NH, 0.f), out_lp, out_lpo, fin_lp;
  HIP_OK(hipMemcpyAsync(out_tok.data(), e->d_tokens.p, out_tok.size() * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(out_len.data(), e->d_seq_len.p, NH * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(out_cum.data(), e->d_cum.p, NH * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(poll, e->d_n_active.p, sizeof(poll), hipMemcpyDeviceToHost, st));
  if (any_sot) HIP_OK(hipMemcpyAsync(ns.data(), e->d_ns.p, NH * 4, hipMemcpyDeviceToHost, st));
  if (rec) {
    out_lp.resize((size_t)NH * C);
    HIP_OK(hipMemcpyAsync(out_lp.data(), e->d_tok_lp.p, out_lp.size() * 4, hipMemcpyDeviceToHost, st));
    if (!beam) {
      out_lpo.resize((size_t)NH * C);
      HIP_OK(hipMemcpyAsync(out_lpo.data(), e->d_tok_lp_o.p, out_lpo.size() * 4, hipMemcpyDeviceToHost, st));
    }
  }
  std::vector<int> fin_tok, fin_len, n_fin;
  std::vector<float> fin_cum;
  if (beam) {
    fin_tok.resize((size_t)W * max_cand * C); fin_len.resize((size_t)W * max_cand); fin_cum.resize((size_t)W * max_cand);
    n_fin.resize(W);
    HIP_OK(hipMemcpyAsync(fin_tok.data(), e->d_fin_tok.p, fin_tok.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(fin_len.data(), e->d_fin_len.p, fin_len.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(fin_cum.data(), e->d_fin_cum.p, fin_cum.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(n_fin.data(), e->d_n_fin.p, W * 4, hipMemcpyDeviceToHost, st));
    if (rec) {
      fin_lp.resize((size_t)W * max_cand * C);
      HIP_OK(hipMemcpyAsync(fin_lp.data(), e->d_fin_lp.p, fin_lp.size() * 4, hipMemcpyDeviceToHost, st));
    }
  }
  HIP_OK(hipStreamSynchronize(st));
  check_decode_error(poll + 1);
  for (int w = 0; w < W; ++w) {
    const int Pw = wa.len[w], h0 = w * per;
    BeamBest best;                              // (lp: the chosen hypothesis' records, from its first generated step)
    const float* best_lpo = nullptr;
    if (beam) {
      const size_t f = (size_t)w * max_cand;
      best = beam_best(a, C, max_cand, Pw, {&fin_tok[f * C], &fin_len[f], &fin_cum[f], rec ? &fin_lp[f * C] : nullptr}, n_fin[w],
                       {&out_tok[(size_t)h0 * C], &out_len[h0], &out_cum[h0], rec ? &out_lp[(size_t)h0 * C] : nullptr});
    } else {
      for (int h = h0; h < h0 + per; ++h) {
        const int n = out_len[h] - Pw;
        const float s = length_norm(a, out_cum[h], n);
        if (s > best.score) {
          best.score = s; best.len = n; best.cum = out_cum[h]; best.tok = &out_tok[(size_t)h * C + Pw];
          if (rec) { best.lp = &out_lp[(size_t)h * C + Pw]; best_lpo = &out_lpo[(size_t)h * C + Pw]; }
        }
      }
    }
    write_window_result(a, wa, w, best.tok, best.len, best.cum, best.score, &ns[h0], best.lp, best_lpo);
  }
  write_stats(a, steps, row_steps, 0, graph.captures);
}

// Row-set decode: greedy (or sampling with one hypothesis) over W windows with at most R = max_rows in flight.
//
// A batch of 30 s windows ends when its LONGEST window does (speech density varies: a few tokens for silence, 200+
// for dense speech), and every decode step pays the weight-streaming GEMM chain however many rows are still live.
// Here the decode keeps a ROW SET: hypothesis slot h of row r holds one window; when the host check finds rows
// whose window ended, it starts the next windows (in h_slots order, which the host sorts longest-expected first)
// in those rows.  The new windows' prompts are prefilled INSIDE that step's decoder pass (pass rows = one decode
// row per live hypothesis + P prompt rows per new one; the final LayerNorm gathers one logits row per row-set row
// in row order), so a refill costs no extra pass.  Rows stay in place while windows wait, so the captured step
// graph stays valid; once the queue is empty and compaction is on, the live rows are packed densely when they
// fall to 7/8 of the pass (row_compact_8ths; re-capture for the new count).  A finished hypothesis' tokens are copied to the
// per-window output tables by the block that ends it (search.hip), since its slot is then reused.
void generate_rows(wm_engine* e, const wm_generate_args* a, const WinArgs& wa, hipStream_t st) {
  const auto& m = e->dm;
  const int C = m.n_text_ctx, V = m.n_vocab;
  const int W = a->n_windows, P = a->prompt_len;
  const int R = a->max_rows > 0 ? std::min(a->max_rows, W) : W;
  const bool rec = a->h_token_logprobs != nullptr;
  // P is the row stride of h_prompts; a window's own values come from wa
  const bool rag = wa.ragged;
  reserve(e, e->n_slots, R);
  // per-window inputs and outputs
  e->d_win_prompt.ensure((size_t)W * P * 4);
  e->d_win_slot.ensure((size_t)W * 4);
  e->d_hyp_out.ensure((size_t)R * 4);
  e->d_res_tok.ensure((size_t)W * C * 4);
  e->d_res_len.ensure((size_t)W * 4);
  e->d_res_cum.ensure((size_t)W * 4);
  e->d_res_ns.ensure((size_t)W * 4);
  if (rec) {
    e->d_tok_lp.ensure((size_t)R * C * 4);
    e->d_tok_lp_o.ensure((size_t)R * C * 4);
    e->d_res_lp.ensure((size_t)W * C * 4);
    e->d_res_lp_o.ensure((size_t)W * C * 4);
  }
  HIP_OK(hipMemcpyAsync(e->d_win_prompt.p, a->h_prompts, (size_t)W * P * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_win_slot.p, a->h_slots, (size_t)W * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(e->d_res_ns.p, 0, (size_t)W * 4, st));
  HIP_OK(hipMemsetAsync(e->d_n_active.p, 0, 4 * 4, st));      // live counter, error word
  {
    std::vector<int> ones(R, 1), ent;          // every slot starts ended (no hypothesis)
    HIP_OK(hipMemcpyAsync(e->d_done.p, ones.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
    lang_assign_windows(e, W, P, st, &ent);
    upload_suppress(e, a, st);                 // (synchronises: `ones` and `ent` go out of scope)
  }
  // pass rows: R decode rows + P prompt rows per starting window; logits rows: R + one sot row per start
  ensure_step(e, R * (1 + wa.Pmax), 2 * R);
  float* logits = e->s_logits.as<float>();
  int* counters = e->d_n_active.as<int>();     // [0] live hypotheses, [1..3] error word
  int* err = counters + 1;
  SearchParams sp = search_params(e, a, logits, P);
  sp.mode = a->temperature > 0.f ? 2 : 0;
  sp.topk = 1;
  sp.row_hyp = e->d_row_hyp.as<int>();
  sp.hyp_out = e->d_hyp_out.as<int>();
  sp.res_tok = e->d_res_tok.as<int>(); sp.res_len = e->d_res_len.as<int>(); sp.res_cum = e->d_res_cum.as<float>();
  if (rag) upload_window_tables(e, wa, R, &sp, nullptr, st);
  // per-window seeds (wm_generate_seeded): the per-window table goes up once, hyp_start copies a window's seed into
  // its slot's row of the selection tables (rows no window has taken yet stay defined, as the ragged tables')
  const bool seeded = sp.mode == 2 && e->call_seeds != nullptr;
  if (seeded) {
    e->d_win_seed.ensure((size_t)W * 8);
    e->d_hyp_seed.ensure((size_t)R * 8);
    e->d_hyp_key.ensure((size_t)R * 4);
    HIP_OK(hipMemcpyAsync(e->d_win_seed.p, e->call_seeds, (size_t)W * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(e->d_hyp_seed.p, 0, (size_t)R * 8, st));
    HIP_OK(hipMemsetAsync(e->d_hyp_key.p, 0, (size_t)R * 4, st));
    sp.hyp_seed = e->d_hyp_seed.as<unsigned long long>(); sp.hyp_key = e->d_hyp_key.as<int>();
  }
  if (rec) {
    sp.tok_lp = e->d_tok_lp.as<float>(); sp.tok_lp_other = e->d_tok_lp_o.as<float>();
    sp.res_lp = e->d_res_lp.as<float>(); sp.res_lp_other = e->d_res_lp_o.as<float>();
  }

  // host view: row r holds hypothesis slot row_hyp[r]; slot h decodes window hyp_win[h] while live[h]
  std::vector<int> row_hyp(R), hyp_win(R, -1);
  std::vector<char> live(R, 0);
  for (int r = 0; r < R; ++r) row_hyp[r] = r;
  RowSet rs;
  rs.W = W; rs.nrows = R;

  // One event pass.  `carry` per new row: the old row index of a carried live row, -1 for a row whose slot starts
  // a window (`starts`, in row order), -2 for an idle row (its slot ended; the selection skips it).
  std::vector<int> carry, new_row_hyp;
  std::vector<std::pair<int, int>> starts;      // (slot, window)
  auto event = [&](hipStream_t s) {
    const int nr = (int)new_row_hyp.size(), nst = (int)starts.size();
    const int nsot = wa.any_sot ? nst : 0;
    int np = 0, n_live = 0, ks = 0;
    for (int c : carry) {
      np += c >= 0 ? 1 : (c == -1 ? wa.len[starts[ks++].second] : 0);
      n_live += c >= -1;
    }
    const EventLists ev(e, np, nr, nsot, nst);
    const EventLists::Ptrs &u = ev.h, &d = ev.d;
    *u.n_live = n_live;
    LangCall* lc = e->call_lang;                // multilingual call: the starting windows' language rows
    if (lc) lc->h_ent.clear();
    int i = 0, k = 0;
    for (int r = 0; r < nr; ++r) {
      u.rh[r] = new_row_hyp[r];
      if (carry[r] >= 0) {
        u.phyp[i] = new_row_hyp[r]; u.psrc[i] = carry[r];
        u.lr[r] = i++;
      } else if (carry[r] == -1) {
        const int h = starts[k].first, w = starts[k].second;
        const int Pw = wa.len[w], sot = wa.sot[w];
        // (a window without a sot index in a call that has some: its row defaults to 0 and its result is dropped)
        for (int p = 0; p < Pw; ++p, ++i) {
          u.ptok[i] = a->h_prompts[(size_t)w * P + p]; u.ppos[i] = p; u.phyp[i] = h; u.psrc[i] = -1;
          if (p == sot) u.lr[nr + k] = i;
          if (lc && p == lc->pos[w]) { lc->h_ent.push_back(i); lc->h_ent.push_back(lc->aidx[w]); }
        }
        u.lr[r] = i - 1;                        // the last prompt position predicts the first token
        u.hs[k] = h; u.ws[k] = w;
        ++k;
      } else {
        u.lr[r] = 0;
      }
    }
    ev.upload(e, s);
    if (lc) lang_assign(e, lc->h_ent, d.ptok, s);
    // carried rows read token / position from the last selection's (old) row order before it is overwritten
    launch_rows_fill(np, d.psrc, d.ptok, d.ppos, e->d_row_tok.as<int>(), e->d_row_pos.as<int>(), s);
    launch_hyp_start(nst, d.hs, d.ws, e->d_win_prompt.as<int>(), P, e->d_win_slot.as<int>(), C, e->d_tokens.as<int>(),
                     e->d_seq_len.as<int>(), e->d_done.as<int>(), e->d_cum.as<float>(), e->d_hyp_slot.as<int>(),
                     e->d_hyp_out.as<int>(), s, rag ? e->d_win_len.as<int>() : nullptr,
                     rag ? e->d_win_maxlen.as<int>() : nullptr, rag ? e->d_hyp_begin.as<int>() : nullptr,
                     rag ? e->d_hyp_maxlen.as<int>() : nullptr,
                     seeded ? e->d_win_seed.as<unsigned long long>() : nullptr,
                     seeded ? e->d_hyp_seed.as<unsigned long long>() : nullptr, seeded ? e->d_hyp_key.as<int>() : nullptr);
    HIP_OK(hipMemcpyAsync(e->d_row_hyp.p, d.rh, (size_t)nr * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(counters, d.n_live, 4, hipMemcpyDeviceToDevice, s));
    decoder_pass(e, np, d.ptok, d.ppos, d.phyp, e->d_done.as<int>(), nullptr, d.lr, nr + nsot, logits, nullptr, 0, nullptr, 1,
                 s, err);
    if (nsot) launch_no_speech(logits + (size_t)nr * V, V, V, nsot, m.no_speech, e->d_res_ns.as<float>(), s, d.ws);
    debug_nan(e, logits, nr, s);
    {
      ProfScope ps(e, P_SELECT, s);
      launch_logits_select(sp, nr, s);
    }
    // host view of the new row set
    for (int r = 0; r < nr; ++r) row_hyp[r] = new_row_hyp[r];
    for (const auto& sw : starts) { hyp_win[sw.first] = sw.second; live[sw.first] = 1; }
    rs.nrows = nr;
  };
  auto step = [&](hipStream_t s) {
    decoder_pass(e, rs.nrows, e->d_row_tok.as<int>(), e->d_row_pos.as<int>(), e->d_row_hyp.as<int>(), e->d_done.as<int>(),
                 nullptr, nullptr, rs.nrows, logits, nullptr, 0, nullptr, 1, s, err);
    debug_nan(e, logits, rs.nrows, s);
    ProfScope ps(e, P_SELECT, s);
    launch_logits_select(sp, rs.nrows, s);
  };
  // a slot whose hypothesis ended is free (its tokens are already in the per-window output tables)
  auto ended = [&](const int* h_done, hipStream_t) {
    int n_live = 0;
    for (int r = 0; r < rs.nrows; ++r) {
      const int h = row_hyp[r];
      if (live[h] && h_done[h]) live[h] = 0;
      n_live += live[h];
    }
    return std::make_pair(n_live, rs.nrows);
  };
  auto rebuild = [&](bool refill) {
    carry.clear(); new_row_hyp.clear(); starts.clear();
    for (int r = 0; r < rs.nrows; ++r) {
      const int h = row_hyp[r];
      if (live[h]) {
        carry.push_back(r); new_row_hyp.push_back(h);
      } else if (refill) {
        if (rs.next < W) {
          carry.push_back(-1); new_row_hyp.push_back(h); starts.push_back({h, rs.next++});
        } else {
          carry.push_back(-2); new_row_hyp.push_back(h);
        }
      }                                         // compact: ended rows leave the row set
    }
    return (int)starts.size();
  };

  RowSetRules rules;
  rules.check = std::max(1, a->check_every);
  rules.refill_min = std::max(1, R / 16);       // a refill pass runs eagerly: batch the starts
  // every window's tokens need at most max_length - P steps
  rules.pass_limit = (long long)(W / std::max(1, R) + 2) * (wa.max_gen + rules.check + 2) + 16;
  rules.compact = a->compact; rules.compact_8ths = row_compact_8ths();
  rules.n_done = R;
  // first pass: the first R windows start
  carry.assign(R, -1);
  new_row_hyp.resize(R);
  for (int r = 0; r < R; ++r) {
    new_row_hyp[r] = r;
    starts.push_back({r, rs.next++});
  }
  StepGraph graph(e, st);
  run_row_set(e, graph, rs, rules, ended, rebuild, event, step);
  graph.finish();

  // ---- results, by window
  std::vector<int> res_tok((size_t)W * C), res_len(W);
  std::vector<float> res_cum(W), res_ns(W), res_lp, res_lpo;
  HIP_OK(hipMemcpyAsync(res_tok.data(), e->d_res_tok.p, res_tok.size() * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(res_len.data(), e->d_res_len.p, (size_t)W * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(res_cum.data(), e->d_res_cum.p, (size_t)W * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(res_ns.data(), e->d_res_ns.p, (size_t)W * 4, hipMemcpyDeviceToHost, st));
  int h_cnt[4] = {0, 0, 0, 0};
  HIP_OK(hipMemcpyAsync(h_cnt, counters, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
  if (rec) {
    res_lp.resize((size_t)W * C);
    res_lpo.resize((size_t)W * C);
    HIP_OK(hipMemcpyAsync(res_lp.data(), e->d_res_lp.p, res_lp.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(res_lpo.data(), e->d_res_lp_o.p, res_lpo.size() * 4, hipMemcpyDeviceToHost, st));
  }
  HIP_OK(hipStreamSynchronize(st));
  check_decode_error(h_cnt + 1);
  for (int w = 0; w < W; ++w)
    write_window_result(a, wa, w, &res_tok[(size_t)w * C], res_len[w], res_cum[w], length_norm(a, res_cum[w], res_len[w]),
                        &res_ns[w], rec ? &res_lp[(size_t)w * C] : nullptr, rec ? &res_lpo[(size_t)w * C] : nullptr);
  write_stats(a, rs.passes, rs.row_steps, rs.refills, graph.captures);
}

// logit_rows (optional): the pass rows whose logits are wanted, in output order (overrides last_only)
// hidden_only: no final LayerNorm and no logits GEMM (d_logits unused); row s * S + p of e->s_x ([rows][n_state] f32)
// then holds the last hidden state of sequence s at position p, on `st`, until the next pass
void forward(wm_engine* e, int n_seq, const int* h_slots, int S, const int* h_tokens, float* d_logits, int last_only,
             const int* h_align, int n_align, float* d_attn, hipStream_t st, const std::vector<int>* logit_rows = nullptr,
             bool hidden_only = false, std::vector<std::vector<int>>* keep = nullptr) {
  check_weights(e);
  const auto& m = e->dm;
  const int C = m.n_text_ctx, H = m.n_head;
  if (S <= 0 || S > C) throw std::runtime_error("forward: bad seq_len");
  reserve(e, e->n_slots, n_seq);
  const int rows = n_seq * S;
  const int nlog = logit_rows ? (int)logit_rows->size() : last_only ? n_seq : rows;
  ensure_step(e, rows, 1);
  std::vector<int> rt(rows), rp(rows), rh(rows), lr(nlog), hs(n_seq), lin((size_t)n_seq * C);
  for (int s = 0; s < n_seq; ++s) {
    if (h_slots[s] < 0 || h_slots[s] >= e->n_slots) throw std::runtime_error("forward: slot out of range");
    hs[s] = h_slots[s];
    for (int p = 0; p < S; ++p) {
      const int r = s * S + p;
      rt[r] = h_tokens[r]; rp[r] = p; rh[r] = s;
    }
    for (int p = 0; p < C; ++p) lin[(size_t)s * C + p] = s;
  }
  for (int i = 0; i < nlog; ++i) lr[i] = logit_rows ? (*logit_rows)[i] : last_only ? i * S + S - 1 : i;
  std::vector<std::vector<int>> amap(m.n_dec_layer, std::vector<int>(H, -1));
  for (int i = 0; i < n_align; ++i) {
    const int l = h_align[2 * i], h = h_align[2 * i + 1];
    if (l < 0 || l >= m.n_dec_layer || h < 0 || h >= H) throw std::runtime_error("forward: bad alignment head");
    amap[l][h] = i;
  }
  e->d_logit_rows.ensure((size_t)nlog * 4);
  HIP_OK(hipMemcpyAsync(e->d_prow_tok.p, rt.data(), rows * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_prow_pos.p, rp.data(), rows * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_prow_hyp.p, rh.data(), rows * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_logit_rows.p, lr.data(), nlog * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_hyp_slot.p, hs.data(), n_seq * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_lin.p, lin.data(), lin.size() * 4, hipMemcpyHostToDevice, st));
  // factored form with capture (alignment): gather the windows' encoder outputs for the per-layer K/V projection
  // (decoder_layer); the rows of a window must reach the teacher-forced kernel (S >= 16, launch_cross_attn)
  e->tf_nwin = 0;
  if (n_align && e->cross_mode == 1 && e->cross_tf && !e->cross_fp8 && S >= 16) {
    const int T = m.n_audio_ctx, d = m.n_state;
    const size_t per = (size_t)T * d;
    e->a_enc.ensure((size_t)n_seq * per * 2);
    e->a_kv.ensure((size_t)2 * n_seq * per * 2);
    const size_t bper = (size_t)xblock_slot_elems(T, d);
    for (int s = 0; s < n_seq; ++s)
      launch_xblock(e->xenc.as<bf16>() + (size_t)hs[s] * bper, 1, T, d, e->a_enc.as<bf16>() + (size_t)s * per, false, st);
    e->tf_nwin = n_seq;
  }
  struct TfReset { wm_engine* e; ~TfReset() { e->tf_nwin = 0; } } tf_reset{e};
  decoder_pass(e, rows, e->d_prow_tok.as<int>(), e->d_prow_pos.as<int>(), e->d_prow_hyp.as<int>(), nullptr,
               e->d_lin.as<int>(), e->d_logit_rows.as<int>(), nlog, hidden_only ? nullptr : d_logits,
               n_align ? &amap : nullptr, n_align, n_align ? d_attn : nullptr, S, st);
  if (keep) {                                   // the caller keeps the uploads' host images alive and waits later
    for (auto* v : {&rt, &rp, &rh, &lr, &hs, &lin}) keep->push_back(std::move(*v));
    return;
  }
  HIP_OK(hipStreamSynchronize(st));
}

// h_rows null: the closed DTW (the path ends at (N, M)); else the open-end form, rows reached to *h_rows
void dtw_run(wm_engine* e, const float* d_x, int N, int M, int* h_i, int* h_j, int* h_len, hipStream_t st,
             int* h_rows = nullptr) {
  if (h_rows && (N <= 0 || M <= 0)) throw std::runtime_error("wm_dtw_open: bad matrix shape");
  e->a_cost.ensure((size_t)(N + 1) * (M + 1) * 4);
  e->a_trace.ensure((size_t)(N + 1) * (M + 1));
  e->a_pi.ensure((size_t)(N + M + 2) * 4);
  e->a_pj.ensure((size_t)(N + M + 2) * 4);
  e->a_plen.ensure(8);                              // path length, rows reached
  int nr[2] = {0, 0};
  if (h_rows)
    launch_dtw_open(d_x, N, M, e->a_cost.as<float>(), e->a_trace.as<signed char>(), e->a_pi.as<int>(),
                    e->a_pj.as<int>(), e->a_plen.as<int>(), e->a_plen.as<int>() + 1, st);
  else
    launch_dtw(d_x, N, M, e->a_cost.as<float>(), e->a_trace.as<signed char>(), e->a_pi.as<int>(), e->a_pj.as<int>(),
               e->a_plen.as<int>(), st);
  HIP_OK(hipMemcpyAsync(nr, e->a_plen.p, h_rows ? 8 : 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  const int n = nr[0];
  if (h_rows) {
    if (nr[1] <= 0) throw std::runtime_error("wm_dtw_open: non-finite alignment cost (item 0)");
    *h_rows = nr[1];
  }
  HIP_OK(hipMemcpyAsync(h_i, e->a_pi.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_j, e->a_pj.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  *h_len = n;
}

// Beam row-set decode: beam search over W windows with at most G = max_rows / K windows (groups of K hypothesis
// slots) in flight.  A group decodes one window; when beam_select ends it (max_cand finished, max_length, or no live
// beam), the host check reads the group's finished list and beams, finalises the window (openai's ranking, as
// generate()) and starts the next window in the group: the event pass prefills the new window's prompt into the
// group's first slot (P rows) beside the other groups' decode rows, and beam_start_kernel resets the group's state.
// The K rows of a group stay together (its window's cross panels are read once for them), the row set keeps its
// groups in place while windows wait (the step graph stays valid), and once nothing waits the finished groups'
// rows are dropped at 7/8 (beam passes are GEMM-row-bound).  No per-step records in this form.
void generate_rows_beam(wm_engine* e, const wm_generate_args* a, const WinArgs& wa, hipStream_t st) {
  const auto& m = e->dm;
  const int C = m.n_text_ctx, V = m.n_vocab;
  const int W = a->n_windows, P = a->prompt_len, K = a->beam_size;
  const int G = std::max(1, std::min(a->max_rows / K, W));
  const int NH = G * K;
  const int max_cand = std::max(1, (int)std::lround(a->beam_size * a->patience));
  if (max_cand > 16) throw std::runtime_error("generate: beam_size * patience must be <= 16");
  if (a->h_token_logprobs) throw std::runtime_error("generate: per-step records need max_rows 0 with beam search");
  // P is the row stride of h_prompts; a window's own values come from wa
  const bool rag = wa.ragged;
  reserve(e, e->n_slots, NH);
  e->d_win_prompt.ensure((size_t)W * P * 4);
  e->d_win_slot.ensure((size_t)W * 4);
  e->d_res_ns.ensure((size_t)W * 4);
  HIP_OK(hipMemcpyAsync(e->d_win_prompt.p, a->h_prompts, (size_t)W * P * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(e->d_win_slot.p, a->h_slots, (size_t)W * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(e->d_res_ns.p, 0, (size_t)W * 4, st));
  HIP_OK(hipMemsetAsync(e->d_n_active.p, 0, 4 * 4, st));
  {
    std::vector<int> ones(NH, 1), ent;         // every group starts ended (no window)
    HIP_OK(hipMemcpyAsync(e->d_done.p, ones.data(), (size_t)NH * 4, hipMemcpyHostToDevice, st));
    lang_assign_windows(e, W, P, st, &ent);
    upload_suppress(e, a, st);                 // (synchronises: `ones` and `ent` go out of scope)
  }
  // pass rows: every hypothesis row + P prompt rows per starting group; logits rows: one per hypothesis row + one
  // sot row per start
  ensure_step(e, NH + G * std::max(wa.Pmax, K), NH + G);
  float* logits = e->s_logits.as<float>();
  int* counters = e->d_n_active.as<int>();
  int* err = counters + 1;
  SearchParams sp = search_params(e, a, logits, P);
  sp.mode = 1; sp.topk = K + 1;
  sp.row_hyp = e->d_row_hyp.as<int>();
  BeamParams bp = beam_params(e, a, sp, max_cand);
  if (rag) upload_window_tables(e, wa, NH, &sp, &bp, st);

  // host view: the row set is a list of groups (K rows each, in order); group g decodes window gwin[g] while glive[g]
  std::vector<int> set(G), gwin(G, -1);
  std::vector<char> glive(G, 0);
  for (int g = 0; g < G; ++g) set[g] = g;
  int nfinal = 0;
  RowSet rs;
  rs.W = W; rs.nrows = NH;
  // the finished groups' lists and beams -> their windows' results (the ranking of generate(): beam_best)
  std::vector<int> f_tok, f_len, f_n, o_tok, o_len;
  std::vector<float> f_cum, o_cum;
  auto finalize = [&](const std::vector<int>& gs, hipStream_t s) {
    if (gs.empty()) return;
    f_tok.resize((size_t)G * max_cand * C); f_len.resize((size_t)G * max_cand); f_cum.resize((size_t)G * max_cand);
    f_n.resize(G); o_tok.resize((size_t)NH * C); o_len.resize(NH); o_cum.resize(NH);
    HIP_OK(hipMemcpyAsync(f_tok.data(), e->d_fin_tok.p, f_tok.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(f_len.data(), e->d_fin_len.p, f_len.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(f_cum.data(), e->d_fin_cum.p, f_cum.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(f_n.data(), e->d_n_fin.p, (size_t)G * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(o_tok.data(), e->d_tokens.p, o_tok.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(o_len.data(), e->d_seq_len.p, (size_t)NH * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(o_cum.data(), e->d_cum.p, (size_t)NH * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    for (int g : gs) {
      const int w = gwin[g], h0 = g * K;
      const size_t f = (size_t)g * max_cand;
      const BeamBest best = beam_best(a, C, max_cand, wa.len[w], {&f_tok[f * C], &f_len[f], &f_cum[f], nullptr}, f_n[g],
                                      {&o_tok[(size_t)h0 * C], &o_len[h0], &o_cum[h0], nullptr});
      // (no-speech values are read once, at the end)
      write_window_result(a, wa, w, best.tok, best.len, best.cum, best.score, nullptr, nullptr, nullptr);
      ++nfinal;
      glive[g] = 0;
      gwin[g] = -1;
    }
  };

  // One event pass: `starts` (group, window) begin in place; `nset` is the new row set (compaction drops groups).
  std::vector<int> nset;
  std::vector<std::pair<int, int>> starts;
  // A starting group's P prompt rows are padded to K with copies of its last prompt row (same hypothesis, position
  // and token: identical self-KV writes), so every group of the pass holds K rows of one window and the
  // cross-attention keeps its per-window grouping (prompts longer than K rows: ungrouped rows).
  // (Prompts of different lengths: ungrouped rows too.)
  const int PR = std::max(wa.Pmax, K);
  const int ev_group = (!rag || wa.same_len) && wa.Pmax <= K ? K : 1;
  auto event = [&](hipStream_t s) {
    const int ng = (int)nset.size(), nr = ng * K, nst = (int)starts.size();
    const int nsot = wa.any_sot ? nst : 0;
    std::vector<int> start_of(G, -1);
    for (int k = 0; k < nst; ++k) start_of[starts[k].first] = k;
    int np = 0, n_live = 0;
    for (int g : nset) {
      np += start_of[g] >= 0 ? (ev_group > 1 ? PR : wa.len[starts[start_of[g]].second]) : K;
      n_live += (start_of[g] >= 0 || glive[g]) ? K : 0;
    }
    const EventLists ev(e, np, nr, nsot, nst);
    const EventLists::Ptrs &u = ev.h, &d = ev.d;
    *u.n_live = n_live;
    LangCall* lc = e->call_lang;                // multilingual call: the starting windows' language rows
    if (lc) lc->h_ent.clear();
    int i = 0, r = 0;
    for (int g : nset) {
      const int h0 = g * K, k = start_of[g];
      if (k >= 0) {
        const int w = starts[k].second;
        int last = 0;
        const int Pw = wa.len[w], sot = wa.sot[w];
        for (int p = 0; p < Pw; ++p, ++i) {
          u.ptok[i] = a->h_prompts[(size_t)w * P + p]; u.ppos[i] = p; u.phyp[i] = h0; u.psrc[i] = -1;
          if (p == sot) u.lr[nr + k] = i;
          if (lc && p == lc->pos[w]) { lc->h_ent.push_back(i); lc->h_ent.push_back(lc->aidx[w]); }
          last = i;
        }
        for (int p = Pw; ev_group > 1 && p < PR; ++p, ++i) {   // (grouped rows: every window has Pw = Pmax <= K)
          u.ptok[i] = a->h_prompts[(size_t)w * P + Pw - 1]; u.ppos[i] = Pw - 1; u.phyp[i] = h0; u.psrc[i] = -1;
          if (lc && Pw - 1 == lc->pos[w]) { lc->h_ent.push_back(i); lc->h_ent.push_back(lc->aidx[w]); }
        }
        for (int b = 0; b < K; ++b, ++r) { u.rh[r] = h0 + b; u.lr[r] = last; }
        u.hs[k] = g; u.ws[k] = w;
      } else {
        for (int b = 0; b < K; ++b, ++i, ++r) {
          u.phyp[i] = h0 + b; u.psrc[i] = h0 + b;
          u.rh[r] = h0 + b; u.lr[r] = i;
        }
      }
    }
    ev.upload(e, s);
    if (lc) lang_assign(e, lc->h_ent, d.ptok, s);
    // carried rows: token / position of their hypothesis from the last beam selection (hypothesis-indexed)
    launch_rows_fill(np, d.psrc, d.ptok, d.ppos, e->d_row_tok.as<int>(), e->d_row_pos.as<int>(), s);
    launch_beam_start(nst, d.hs, d.ws, K, e->d_win_prompt.as<int>(), P, e->d_win_slot.as<int>(), C, e->d_tokens.as<int>(),
                      e->d_lin.as<int>(), e->d_seq_len.as<int>(), e->d_done.as<int>(), e->d_cum.as<float>(),
                      e->d_hyp_slot.as<int>(), e->d_n_fin.as<int>(), s, rag ? e->d_win_len.as<int>() : nullptr,
                      rag ? e->d_win_maxlen.as<int>() : nullptr, rag ? e->d_hyp_begin.as<int>() : nullptr,
                      rag ? e->d_hyp_maxlen.as<int>() : nullptr);
    HIP_OK(hipMemcpyAsync(e->d_row_hyp.p, d.rh, (size_t)nr * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(counters, d.n_live, 4, hipMemcpyDeviceToDevice, s));
    decoder_pass(e, np, d.ptok, d.ppos, d.phyp, e->d_done.as<int>(), e->d_lin.as<int>(), d.lr, nr + nsot, logits, nullptr, 0,
                 nullptr, ev_group, s, err);
    if (nsot) launch_no_speech(logits + (size_t)nr * V, V, V, nsot, m.no_speech, e->d_res_ns.as<float>(), s, d.ws);
    debug_nan(e, logits, nr, s);
    {
      ProfScope ps(e, P_SELECT, s);
      launch_logits_select(sp, nr, s);
      launch_beam_select(bp, G, s);
    }
    for (const auto& gw : starts) { gwin[gw.first] = gw.second; glive[gw.first] = 1; }
    set = nset;
    rs.nrows = nr;
  };
  auto step = [&](hipStream_t s) {
    launch_rows_fill(rs.nrows, e->d_row_hyp.as<int>(), e->d_prow_tok.as<int>(), e->d_prow_pos.as<int>(),
                     e->d_row_tok.as<int>(), e->d_row_pos.as<int>(), s);
    decoder_pass(e, rs.nrows, e->d_prow_tok.as<int>(), e->d_prow_pos.as<int>(), e->d_row_hyp.as<int>(), e->d_done.as<int>(),
                 e->d_lin.as<int>(), nullptr, rs.nrows, logits, nullptr, 0, nullptr, K, s, err);
    debug_nan(e, logits, rs.nrows, s);
    ProfScope ps(e, P_SELECT, s);
    launch_logits_select(sp, rs.nrows, s);
    launch_beam_select(bp, G, s);
  };
  // a group whose window beam_select ended is finalised and free
  auto ended = [&](const int* h_done, hipStream_t s) {
    std::vector<int> gs;
    for (int g = 0; g < G; ++g)
      if (glive[g] && h_done[g * K]) gs.push_back(g);
    finalize(gs, s);
    int n_live = 0;
    for (int g : set) n_live += glive[g];
    return std::make_pair(n_live, (int)set.size());
  };
  auto rebuild = [&](bool refill) {
    nset.clear(); starts.clear();
    for (int g : set) {
      if (glive[g]) nset.push_back(g);
      else if (refill && rs.next < W) { nset.push_back(g); starts.push_back({g, rs.next++}); }
      else if (refill) nset.push_back(g);       // idle until compaction (rows stay in place)
    }
    return (int)starts.size();
  };

  RowSetRules rules;
  rules.check = std::max(1, a->check_every);
  rules.refill_min = std::max(1, G / 16);
  rules.pass_limit = (long long)(W / G + 2) * (wa.max_gen + rules.check + 2) + 16;
  rules.compact = a->compact; rules.compact_8ths = 7;   // opt-in, as the header says; beam passes are GEMM-row-bound
  rules.n_done = NH;
  nset = set;
  for (int g = 0; g < G; ++g) starts.push_back({g, rs.next++});
  StepGraph graph(e, st);
  run_row_set(e, graph, rs, rules, ended, rebuild, event, step);
  graph.finish();
  std::vector<float> res_ns(W);
  int h_cnt[4] = {0, 0, 0, 0};
  HIP_OK(hipMemcpyAsync(res_ns.data(), e->d_res_ns.p, (size_t)W * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_cnt, counters, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  check_decode_error(h_cnt + 1);
  if (nfinal != W) throw std::runtime_error("generate: beam row-set finished " + std::to_string(nfinal) + " of " +
                                            std::to_string(W) + " windows");
  for (int w = 0; w < W; ++w)
    if (a->h_no_speech) a->h_no_speech[w] = wa.sot[w] >= 0 ? res_ns[w] : 0.f;
  write_stats(a, rs.passes, rs.row_steps, rs.refills, graph.captures);
}

void align(wm_engine* e, int slot, int sot_len, const int* h_sot, int n_text, const int* h_text, int num_frames,
           const int* h_heads, int n_heads, int medw, float* h_probs, int* h_ti, int* h_tj, int* h_len, hipStream_t st) {
  const auto& m = e->dm;
  const int T = m.n_audio_ctx, V = m.n_vocab;
  const int S = sot_len + 1 + n_text + 1;
  if (n_text <= 0 || S > m.n_text_ctx) throw std::runtime_error("wm_align: bad token count");
  const int F = num_frames / 2;
  if (F <= 0 || F > T) throw std::runtime_error("wm_align: bad num_frames");
  std::vector<int> toks(S), next(n_text);
  for (int i = 0; i < sot_len; ++i) toks[i] = h_sot[i];
  toks[sot_len] = m.no_timestamps;
  for (int i = 0; i < n_text; ++i) toks[sot_len + 1 + i] = next[i] = h_text[i];
  toks[S - 1] = m.eot;
  e->a_logits.ensure((size_t)S * V * 4);
  e->a_attn.ensure((size_t)S * n_heads * T * 4);
  forward(e, 1, &slot, S, toks.data(), e->a_logits.as<float>(), 0, h_heads, n_heads, e->a_attn.as<float>(), st);
  // text token probabilities: position sot_len + k predicts text token k
  e->a_next.ensure((size_t)n_text * 4);
  e->a_probs.ensure((size_t)n_text * 4);
  HIP_OK(hipMemcpyAsync(e->a_next.p, next.data(), n_text * 4, hipMemcpyHostToDevice, st));
  launch_token_probs(e->a_logits.as<float>() + (size_t)sot_len * V, n_text, V, m.eot, e->a_next.as<int>(),
                     e->a_probs.as<float>(), st);
  // DTW input matrix rows sot_len .. S-2 (n_text + 1 rows)
  const int nrows = n_text + 1;
  e->a_rowsum.ensure((size_t)S * n_heads * 4);
  e->a_z.ensure((size_t)n_heads * S * F * 4);
  e->a_mat.ensure((size_t)nrows * F * 4);
  launch_align_matrix(e->a_attn.as<float>(), S, n_heads, T, F, medw, sot_len, nrows, e->a_rowsum.as<float>(),
                      e->a_z.as<float>(), e->a_mat.as<float>(), st);
  HIP_OK(hipMemcpyAsync(h_probs, e->a_probs.p, n_text * 4, hipMemcpyDeviceToHost, st));
  dtw_run(e, e->a_mat.as<float>(), nrows, F, h_ti, h_tj, h_len, st);
}

// Batched word alignment (ctranslate2 Whisper.align over a batch of windows [FW↑]): items are chunked so the
// captured attention (S x heads x 1500 f32 per item) and the text-row logits stay under ~1.5 GB; per chunk ONE
// teacher-forced decoder pass over every item (sequences padded with <|endoftext|> to the chunk's longest: the
// pass is causal, so padding never changes a real position), then per item the probabilities and the
// alignment matrix, and one batched DTW launch for the whole chunk.
// h_rows null: wm_align_batch (every path ends at its matrix' last row).  h_rows [n]: wm_align_open_batch, the same
// pass, capture, probabilities and matrices with the open-end batched DTW; item i's rows reached go to h_rows[i],
// and an item whose minimum end cost is not finite fails the call.
void align_batch(wm_engine* e, int n, const int* h_slots, int sot_len, const int* h_sot, const int* h_text_off,
                 const int* h_text, const int* h_num_frames, const int* h_heads, int n_heads, int medw, float* h_probs,
                 const long long* h_path_off, int* h_pi, int* h_pj, int* h_plen, hipStream_t st, int* h_rows = nullptr) {
  const auto& m = e->dm;
  const int T = m.n_audio_ctx, V = m.n_vocab;
  const std::string who = h_rows ? "wm_align_open_batch" : "wm_align_batch";
  if (n <= 0) return;
  if (n_heads <= 0) throw std::runtime_error(who + ": no alignment heads");
  std::vector<int> S(n), nt(n), F(n);
  for (int i = 0; i < n; ++i) {
    nt[i] = h_text_off[i + 1] - h_text_off[i];
    S[i] = sot_len + 1 + nt[i] + 1;
    F[i] = h_num_frames[i] / 2;
    if (nt[i] <= 0 || S[i] > m.n_text_ctx) throw std::runtime_error(who + ": bad token count");
    if (F[i] <= 0 || F[i] > T) throw std::runtime_error(who + ": bad num_frames");
  }
  // The capture buffer (S x heads x 1500 f32 per item: ~230 MB for a large-v3 window with the default 320 heads)
  // may take half of the free device memory (at most 48 GB): a batch of 150 large-v3 windows then aligns in ONE
  // teacher-forced pass instead of ~25 passes of 6 windows under a fixed 1.5 GB budget (round 3: 0.89 s per
  // 150-window step, most of it those passes).
  size_t free_b = 0, total_b = 0;
  HIP_OK(hipMemGetInfo(&free_b, &total_b));
  // the factored form's alignment pass also gathers each item's encoder output and its per-layer K/V projection
  // (a_enc + a_kv, 3 x T x d bf16 per item, forward()): counted per item below
  const bool tf_gather = e->cross_mode == 1 && e->cross_tf && !e->cross_fp8;
  const double per_item_kv = tf_gather ? 3.0 * (double)T * m.n_state * 2 : 0.0;
  const double reusable = (double)e->a_attn.bytes + (double)e->a_logits.bytes +
                          (tf_gather ? (double)e->a_enc.bytes + (double)e->a_kv.bytes : 0.0);
  const double budget = std::max(1.5e9, std::min(48e9, 0.5 * (double)free_b + reusable));
  static const bool align_log = [] {
    const char* v = std::getenv("VLOG_AMD_ALIGN_LOG");
    return v && v[0] == '1';
  }();
  if (align_log) std::fprintf(stderr, "[align_batch] %d items, free %.1f GB, budget %.1f GB\n", n, free_b / 1e9, budget / 1e9);
  // Items longest-first, chunked so padding (every sequence of a chunk padded to its longest) stays under a
  // quarter of the chunk's rows: with transcripts of 5 to 220 tokens one padded pass would run ~2x the rows.
  std::vector<int> ord(n);
  for (int i = 0; i < n; ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return S[x] > S[y]; });
  int i0 = 0;
  while (i0 < n) {
    int i1 = i0, smax = 0;
    long long ntext = 0, sum_s = 0;
    while (i1 < n) {
      const int it = ord[i1];
      const int s2 = std::max(smax, S[it]);
      // per item: its attention capture, the factored form's K/V gather, and the fused alignment's f64 statistics
      // (n_heads x F x 2 doubles, F <= T: the buffer is c x n_heads x fmax x 16 bytes)
      const double bytes = (double)(i1 - i0 + 1) * (s2 * n_heads * T * 4 + per_item_kv + (double)n_heads * T * 16) +
                           (double)(ntext + nt[it]) * V * 4;
      if (i1 > i0 && (bytes > budget || (double)(i1 - i0 + 1) * s2 > 1.25 * (double)(sum_s + S[it]))) break;
      smax = s2;
      ntext += nt[it];
      sum_s += S[it];
      ++i1;
    }
    const int c = i1 - i0;
    std::vector<int> toks((size_t)c * smax, m.eot), slots(c), lrows, next;
    for (int k = 0; k < c; ++k) {
      const int i = ord[i0 + k];
      int* t = &toks[(size_t)k * smax];
      for (int j = 0; j < sot_len; ++j) t[j] = h_sot[j];
      t[sot_len] = m.no_timestamps;
      for (int j = 0; j < nt[i]; ++j) {
        t[sot_len + 1 + j] = h_text[h_text_off[i] + j];
        lrows.push_back(k * smax + sot_len + j);         // position sot_len + j predicts text token j
        next.push_back(h_text[h_text_off[i] + j]);
      }
      slots[k] = h_slots[i];
    }
    e->a_logits.ensure((size_t)ntext * V * 4);
    e->a_attn.ensure((size_t)c * smax * n_heads * T * 4);
    forward(e, c, slots.data(), smax, toks.data(), e->a_logits.as<float>(), 0, h_heads, n_heads, e->a_attn.as<float>(), st,
            &lrows);
    e->a_next.ensure((size_t)ntext * 4);
    e->a_probs.ensure((size_t)ntext * 4);
    HIP_OK(hipMemcpyAsync(e->a_next.p, next.data(), ntext * 4, hipMemcpyHostToDevice, st));
    launch_token_probs(e->a_logits.as<float>(), (int)ntext, V, m.eot, e->a_next.as<int>(), e->a_probs.as<float>(), st);
    // alignment matrices of the chunk, packed; DTW scratch and path offsets
    std::vector<long long> xo(c), co(c), po(c);
    std::vector<int> Ns(c), Ms(c);
    long long xt = 0, ct = 0, pt = 0;
    for (int k = 0; k < c; ++k) {
      const int i = ord[i0 + k];
      Ns[k] = nt[i] + 1; Ms[k] = F[i];
      xo[k] = xt; co[k] = ct; po[k] = pt;
      xt += (long long)Ns[k] * Ms[k];
      ct += (long long)(Ns[k] + 1) * (Ms[k] + 1);
      pt += Ns[k] + Ms[k];
    }
    e->a_mat.ensure((size_t)xt * 4);
    e->a_meta.ensure((size_t)c * (3 * 8 + 3 * 4));
    char* meta = (char*)e->a_meta.p;
    long long* d_xo = (long long*)meta;
    long long* d_co = d_xo + c;
    long long* d_po = d_co + c;
    int* d_N = (int*)(d_po + c);
    int* d_M = d_N + c;
    int* d_S = d_M + c;
    std::vector<int> Ss(c);
    int fmax = 0, nmax = 0;
    for (int k = 0; k < c; ++k) {
      Ss[k] = S[ord[i0 + k]];
      fmax = std::max(fmax, Ms[k]);
      nmax = std::max(nmax, Ns[k]);
    }
    HIP_OK(hipMemcpyAsync(d_xo, xo.data(), c * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_co, co.data(), c * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_po, po.data(), c * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_N, Ns.data(), c * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_M, Ms.data(), c * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_S, Ss.data(), c * 4, hipMemcpyHostToDevice, st));
    if (align_get_fused()) {
      // the whole chunk in three launches (rows of window k: its text + <|endoftext|>, from row sot_len)
      e->a_rowsum.ensure((size_t)c * smax * n_heads * 4);
      e->a_z.ensure((size_t)c * n_heads * fmax * 16);
      launch_align_matrix_batch(e->a_attn.as<float>(), c, smax, n_heads, T, fmax, nmax, medw, sot_len, d_S, d_M, d_N, d_xo,
                                e->a_rowsum.as<float>(), (double*)e->a_z.p, e->a_mat.as<float>(), st);
    } else {
      e->a_rowsum.ensure((size_t)smax * n_heads * 4);
      e->a_z.ensure((size_t)n_heads * smax * T * 4);
      for (int k = 0; k < c; ++k) {
        const int i = ord[i0 + k];
        launch_align_matrix(e->a_attn.as<float>() + (size_t)k * smax * n_heads * T, S[i], n_heads, T, F[i], medw, sot_len,
                            nt[i] + 1, e->a_rowsum.as<float>(), e->a_z.as<float>(), e->a_mat.as<float>() + xo[k], st);
      }
    }
    e->a_cost.ensure((size_t)ct * 4);
    e->a_trace.ensure((size_t)ct);
    e->a_pi.ensure((size_t)pt * 4);
    e->a_pj.ensure((size_t)pt * 4);
    e->a_plen.ensure((size_t)c * 8);                 // path lengths [c], then rows reached [c]
    if (h_rows)
      launch_dtw_open_batch(e->a_mat.as<float>(), d_xo, d_N, d_M, e->a_cost.as<float>(), e->a_trace.as<signed char>(),
                            d_co, e->a_pi.as<int>(), e->a_pj.as<int>(), d_po, e->a_plen.as<int>(),
                            e->a_plen.as<int>() + c, c, st);
    else
      launch_dtw_batch(e->a_mat.as<float>(), d_xo, d_N, d_M, e->a_cost.as<float>(), e->a_trace.as<signed char>(), d_co,
                       e->a_pi.as<int>(), e->a_pj.as<int>(), d_po, e->a_plen.as<int>(), c, st);
    std::vector<int> pi(pt), pj(pt), plen(h_rows ? 2 * c : c);
    std::vector<float> probs(ntext);                // in chunk order: item k's text tokens after item k-1's
    HIP_OK(hipMemcpyAsync(probs.data(), e->a_probs.p, ntext * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(pi.data(), e->a_pi.p, pt * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(pj.data(), e->a_pj.p, pt * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(plen.data(), e->a_plen.p, plen.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int k = 0, pos = 0; k < c; ++k) {
      const int i = ord[i0 + k];
      if (h_rows) {
        if (plen[c + k] <= 0) throw std::runtime_error(who + ": non-finite alignment cost (item " + std::to_string(i) + ")");
        h_rows[i] = plen[c + k];
      }
      for (int j = 0; j < nt[i]; ++j) h_probs[h_text_off[i] + j] = probs[pos + j];
      pos += nt[i];
      h_plen[i] = plen[k];
      for (int q = 0; q < plen[k]; ++q) {
        h_pi[h_path_off[i] + q] = pi[po[k] + q];
        h_pj[h_path_off[i] + q] = pj[po[k] + q];
      }
    }
    i0 = i1;
  }
}

template <class F>
int guarded(wm_engine* e, F&& f) {
  try {
    if (!e) throw std::runtime_error("null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    struct GenScope {                     // restored on every exit, exceptions included
      long long* prev;
      explicit GenScope(long long* g) : prev(t_realloc) { t_realloc = g; }
      ~GenScope() { t_realloc = prev; }
    } gs(&e->realloc_gen);
    HIP_OK(hipSetDevice(e->device));
    f();
    return 0;
  } catch (const std::exception& ex) {
    g_err = ex.what();
    return -1;
  }
}

// The model entry points need every weight slot set (an engine made for the front end alone has none)
void require_weights(wm_engine* e) {
  if (e->weights_ok) return;
  for (auto& kv : e->slots)
    if (!kv.second.set) throw std::runtime_error("engine weights incomplete (front-end-only engine?): " + kv.first);
  e->weights_ok = true;
}

// cross_mode / cross_fp8 / cross_kv_fp8: switching re-allocates the window slots in the new form (their contents are dropped: run
// wm_cross_kv again)
void set_cross_form(wm_engine* e, int* field, int v) {
  if (v == *field) return;
  HIP_OK(hipDeviceSynchronize());
  *field = v;
  const int n = e->n_slots;
  e->n_slots = 0;
  if (n > 0) reserve(e, n, e->n_hyp_cap);
  else { e->ckv.release(); e->ckv_exp.release(); e->kv8_stage.release(); e->xenc.release(); e->xscale.release(); }
}

void set_cross_kv_fp8(wm_engine* e, int64_t v) {
  if (v < 0 || v > 2) throw std::runtime_error("wm_set_option: cross_kv_fp8 is 0 (bf16 panels), 1 (fp8 panels) or 2 (reference form)");
  set_cross_form(e, &e->cross_kv_fp8, (int)v);
}

void set_dec_plan_preset(wm_engine* e, int64_t v) {
  if (v != 0 && v != 1) throw std::runtime_error("wm_set_option: decode_gemm_plan is 0 or 1");
  for (int i = 0; i < DEC_NPROJ; ++i) e->dec_plan[i] = kDecPlanPresets[v][i], e->dec_cols[i] = kDecColsPresets[v][i];
}

int64_t get_dec_plan_preset(wm_engine* e) {
  for (int q = 0; q < 2; ++q) {
    bool eq = true;
    for (int i = 0; i < DEC_NPROJ; ++i) eq &= e->dec_plan[i] == kDecPlanPresets[q][i] && e->dec_cols[i] == kDecColsPresets[q][i];
    if (eq) return q;
  }
  return -1;                                    // a per-projection setting departs from both presets
}

int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return std::max(lo, std::min(v, hi)); }

// The scalar engine options, one row each: the wm_set_option / wm_get_option key, the environment variable that
// overrides the default at wm_create (nullptr: none), a getter and a validating setter.  wm_create passes atoi of
// every environment variable that is set to the same setter, so a value the setter rejects fails wm_create with
// the setter's message.  The per-projection forms ("decode_gemm.<proj>", "decode_gemm_cols.<proj>" and the
// VLOG_AMD_DEC_GEMM / _COLS / _KR lists) are handled beside the table.  include/whisper_mi355.h documents exactly
// these keys (tests/test_option_docs.py).
struct OptRow {
  const char* key;
  const char* env;
  int64_t (*get)(wm_engine*);
  void (*set)(wm_engine*, int64_t);
};
#define OPT_GET(expr) [](wm_engine* e) -> int64_t { return expr; }
#define OPT_SET(stmt) [](wm_engine* e, int64_t v) { stmt; }
const OptRow kOptions[] = {
    {"decode_split", "VLOG_AMD_DEC_SPLIT", OPT_GET(e->dec_split), OPT_SET(e->dec_split = v != 0)},
    {"decode_graph", "VLOG_AMD_DEC_GRAPH", OPT_GET(e->dec_graph), OPT_SET(e->dec_graph = v != 0)},
    {"decode_gemv", "VLOG_AMD_DEC_GEMV", OPT_GET(e->dec_gemv), OPT_SET(e->dec_gemv = v != 0)},
    {"decode_gemv_ln", "VLOG_AMD_DEC_GEMV_LN", OPT_GET(e->dec_gemv_ln), OPT_SET(e->dec_gemv_ln = v != 0)},
    {"decode_gemv_ln_fc2", nullptr, OPT_GET(e->dec_gemv_ln_fc2), OPT_SET(e->dec_gemv_ln_fc2 = v != 0)},
    {"decode_ring_gemm", "VLOG_AMD_DEC_RING", OPT_GET(e->dec_ring), OPT_SET(e->dec_ring = v != 0)},
    {"decode_gemm_plan", "VLOG_AMD_DEC_PLAN", get_dec_plan_preset, set_dec_plan_preset},
    {"decode_gemm_big_rows", "VLOG_AMD_DEC_BIG_ROWS", OPT_GET(e->dec_big_rows),
     OPT_SET(e->dec_big_rows = (int)clamp64(v, 0, 1 << 20))},
    {"decode_gemm_big128", "VLOG_AMD_DEC_BIG128", OPT_GET(e->dec_big128), OPT_SET(e->dec_big128 = (int)clamp64(v, 0, 1 << 20))},
    {"decode_gemm_big_fc2_kr", nullptr, OPT_GET(e->dec_big_fc2_kr),
     OPT_SET(if (v != 0 && (v < 64 || v % 64 != 0)) throw std::runtime_error("decode_gemm_big_fc2_kr: 0 or a multiple of 64");
             e->dec_big_fc2_kr = (int)std::min<int64_t>(v, 1 << 20))},
    {"decode_gemm_big_lds", "VLOG_AMD_DEC_BIG_LDS", OPT_GET(e->dec_big_lds),
     OPT_SET(if (v != 72 && v != 144) throw std::runtime_error("decode_gemm_big_lds: 72 or 144"); e->dec_big_lds = (int)v)},
    {"cross_mode", "VLOG_AMD_CROSS_MODE", OPT_GET(e->cross_mode), OPT_SET(set_cross_form(e, &e->cross_mode, v ? 1 : 0))},
    {"cross_fp8", "VLOG_AMD_CROSS_FP8", OPT_GET(e->cross_fp8), OPT_SET(set_cross_form(e, &e->cross_fp8, v ? 1 : 0))},
    {"cross_kv_fp8", "VLOG_AMD_CROSS_KV_FP8", OPT_GET(e->cross_kv_fp8), OPT_SET(set_cross_kv_fp8(e, v))},
    {"cross_attn_blocks", "VLOG_AMD_CROSS_BLOCKS", OPT_GET(e->cross_cap), OPT_SET(e->cross_cap = (int)clamp64(v, 0, INT32_MAX))},
    {"cross_attn_fuse", "VLOG_AMD_CROSS_FUSE", OPT_GET(e->cross_fuse), OPT_SET(e->cross_fuse = (int)(v & 3))},
    {"cross_attn_snake", "VLOG_AMD_XSNAKE", OPT_GET(e->xsnake), OPT_SET(e->xsnake = v != 0)},
    {"cross_attn_keep", "VLOG_AMD_XKEEP", OPT_GET(e->xkeep), OPT_SET(e->xkeep = (int)clamp64(v, 0, 1 << 20))},
    {"cross_tf", nullptr, OPT_GET(e->cross_tf), OPT_SET(e->cross_tf = v ? 1 : 0)},
    {"cross_mfma", nullptr, OPT_GET(e->cross_mfma), OPT_SET(e->cross_mfma = v ? 1 : 0)},
    {"cross_mfma_fuse", nullptr, OPT_GET(e->cross_mfma_fuse), OPT_SET(e->cross_mfma_fuse = v ? 1 : 0)},
    {"encode_chunk", "VLOG_AMD_ENC_CHUNK", OPT_GET(e->enc_chunk), OPT_SET(e->enc_chunk = (int)clamp64(v, 1, 4096))},
    {"gemm_persistent", nullptr, OPT_GET(gemm_8p_get_persistent()), OPT_SET(gemm_8p_set_persistent((int)v))},
    {"align_fused", nullptr, OPT_GET(align_get_fused()), OPT_SET(align_set_fused((int)v))},
    {"debug_nan_row", nullptr, OPT_GET(e->dbg_nan_row), OPT_SET(e->dbg_nan_row = (int)clamp64(v, -1, 1 << 30))},
    {"debug_nan_count", nullptr, OPT_GET(e->dbg_nan_count), OPT_SET(e->dbg_nan_count = (int)clamp64(v, 1, 1 << 20))},
};
#undef OPT_GET
#undef OPT_SET

const OptRow* find_option(const std::string& key) {
  for (const OptRow& r : kOptions)
    if (key == r.key) return &r;
  return nullptr;
}

// "decode_gemm.<proj>" / "decode_gemm_cols.<proj>": the engine's per-projection entry, or nullptr for any other key
int* dec_proj_option(wm_engine* e, const std::string& k, const char* who, bool* is_cols) {
  const bool cols = k.rfind("decode_gemm_cols.", 0) == 0;
  if (!cols && k.rfind("decode_gemm.", 0) != 0) return nullptr;
  const std::string pj = k.substr(cols ? 17 : 12);
  for (int i = 0; i < DEC_NPROJ; ++i)
    if (pj == kDecProjNames[i]) {
      *is_cols = cols;
      return cols ? &e->dec_cols[i] : &e->dec_plan[i];
    }
  throw std::runtime_error(std::string(who) + ": unknown projection " + pj);
}

// ---- sample-rate conversion to 16 kHz (wm_resample*): the plan and the f64 taps of the definition in
// include/whisper_mi355.h (scipy.signal.resample_poly's default filter), pure host
struct RsPlan {
  int up, down, half;
};
constexpr int kRsMaxTaps = 16384;

RsPlan rs_plan(int32_t rate, const char* who) {
  if (rate <= 0) throw std::runtime_error(std::string(who) + ": unsupported sample rate " + std::to_string(rate) + " Hz");
  int a = 16000, b = rate;
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  RsPlan p{16000 / a, rate / a, 0};
  if (p.up == 1 && p.down == 1) return p;              // the identity: one tap of 1, downmix only
  const long long m = std::max(p.up, p.down);
  if (20 * m + 1 > kRsMaxTaps)
    throw std::runtime_error(std::string(who) + ": unsupported sample rate " + std::to_string(rate) + " Hz: 16000/" +
                             std::to_string(rate) + " = " + std::to_string(p.up) + "/" + std::to_string(p.down) +
                             " needs " + std::to_string(20 * m + 1) + " filter taps (at most " +
                             std::to_string(kRsMaxTaps) + ")");
  p.half = (int)(10 * m);
  return p;
}

// I0 on [0, 5] by its power series sum_k ((x/2)^2)^k / (k!)^2 (terms fall below 1e-18 of the sum within 30)
double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 64 && term > 1e-18 * sum; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
  }
  return sum;
}

std::vector<double> rs_taps_f64(const RsPlan& p) {
  if (p.half == 0) return {1.0};
  const int m = std::max(p.up, p.down), n = 2 * p.half + 1;
  const double pi = 3.14159265358979323846, i0b = bessel_i0(5.0);
  std::vector<double> h(n);
  double sum = 0.0;
  for (int k = 0; k < n; ++k) {
    const double u = (double)(k - p.half), x = u / m, r = u / p.half;
    const double s = u == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
    h[k] = s / m * (bessel_i0(5.0 * std::sqrt(1.0 - r * r)) / i0b);
    sum += h[k];
  }
  for (double& v : h) v = v / sum * p.up;
  return h;
}

// The ratio's f32 taps on the device in polyphase order, pp[q * T + t] = h[q + t up] (zero where q + t up > 2 half;
// the kernel reads none of those)
const float* rs_device_taps(wm_engine* e, const RsPlan& p, int* T) {
  auto& c = e->rs_taps[{p.up, p.down}];
  if (!c.pp.p) {
    const std::vector<double> h = rs_taps_f64(p);
    // row stride: the taps per phase, made odd so that the lanes of a wave (each on its own phase q) spread over
    // the LDS banks (44.1 kHz: 56 taps per phase put every lane on one of four banks)
    const int n = (int)h.size(), t = ((n + p.up - 1) / p.up) | 1;
    std::vector<float> pp((size_t)p.up * t, 0.f);
    for (int k = 0; k < n; ++k) pp[(size_t)(k % p.up) * t + k / p.up] = (float)h[k];
    c.pp.ensure(pp.size() * sizeof(float));
    HIP_OK(hipMemcpy(c.pp.p, pp.data(), pp.size() * sizeof(float), hipMemcpyHostToDevice));
    c.T = t;
  }
  *T = c.T;
  return c.pp.as<float>();
}

inline long long ceil_div(long long a, long long b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }   // b > 0

}  // namespace

extern "C" {

const char* wm_last_error(void) { return g_err.c_str(); }
int32_t wm_abi_version(void) { return 4; }

int wm_create(const wm_model_dims* dims, int32_t device, wm_engine** out) {
  try {
    if (!dims || !out) throw std::runtime_error("wm_create: null argument");
    *out = nullptr;
    if (dims->n_head <= 0 || dims->n_state <= 0 || dims->n_mels <= 0 || dims->n_enc_layer <= 0 ||
        dims->n_dec_layer <= 0 || dims->n_vocab <= 0 || dims->n_text_ctx <= 0 || dims->n_text_ctx > 448)
      throw std::runtime_error("wm_create: dimensions must be positive (n_text_ctx <= 448)");
    for (int32_t t : {dims->eot, dims->sot, dims->no_speech, dims->no_timestamps, dims->timestamp_begin, dims->blank})
      if (t < 0 || t >= dims->n_vocab) throw std::runtime_error("wm_create: special token id out of the vocabulary");
    if (dims->n_state % 64 != 0 || dims->n_state / dims->n_head != 64)
      throw std::runtime_error("wm_create: head_dim must be 64 and n_state a multiple of 64");
    if (dims->n_audio_ctx != 1500) throw std::runtime_error("wm_create: n_audio_ctx must be 1500");
    HIP_OK(hipSetDevice(device));
    auto* e = new wm_engine();
    e->dm = *dims;
    e->device = device;
    try {
      // environment overrides of the defaults, through the options' own setters (kOptions)
      for (const OptRow& r : kOptions)
        if (const char* v = r.env ? std::getenv(r.env) : nullptr) r.set(e, std::atoi(v));
      // per projection, after the preset: e.g. VLOG_AMD_DEC_GEMM="qkv=32,fc2=64" (rows per block),
      // VLOG_AMD_DEC_COLS="fc1=64"
      auto per_proj = [](const char* v, int* dst) {
        std::string spec(v);
        size_t pos = 0;
        while (pos < spec.size()) {
          const size_t end = std::min(spec.find(',', pos), spec.size());
          const std::string item = spec.substr(pos, end - pos);
          const size_t eq = item.find('=');
          if (eq != std::string::npos)
            for (int i = 0; i < DEC_NPROJ; ++i)
              if (item.substr(0, eq) == kDecProjNames[i]) dst[i] = std::atoi(item.c_str() + eq + 1);
          pos = end + 1;
        }
      };
      if (const char* v = std::getenv("VLOG_AMD_DEC_GEMM")) per_proj(v, e->dec_plan);
      if (const char* v = std::getenv("VLOG_AMD_DEC_COLS")) per_proj(v, e->dec_cols);
      if (const char* v = std::getenv("VLOG_AMD_DEC_KR")) per_proj(v, e->dec_kr);
      build_layout(e);
      build_frontend(e, nullptr);
    } catch (...) {
      delete e;
      throw;
    }
    *out = e;
    return 0;
  } catch (const std::exception& ex) {
    g_err = ex.what();
    return -1;
  }
}

void wm_destroy(wm_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  for (DevBuf* b : {&e->arena, &e->fe_window, &e->fe_cos, &e->fe_sin, &e->fe_filt, &e->fe_lo, &e->fe_hi, &e->e_cols,
                    &e->e_h1, &e->e_x, &e->e_hb, &e->e_qkv, &e->e_ao, &e->e_ff, &e->e_seek, &e->e_len, &e->ckv,
                    &e->ckv_exp, &e->kv8_stage, &e->skv, &e->d_tokens, &e->d_lin, &e->d_seq_len, &e->d_done, &e->d_cum, &e->d_row_tok,
                    &e->d_row_pos, &e->d_row_hyp, &e->d_hyp_slot, &e->d_n_active, &e->d_suppress, &e->d_cand_tok,
                    &e->d_cand_lp, &e->d_fin_tok, &e->d_fin_len, &e->d_fin_cum, &e->d_n_fin, &e->d_ns,
                    &e->d_logit_rows, &e->d_prow_tok, &e->d_prow_pos, &e->d_prow_hyp, &e->d_head_map, &e->s_x,
                    &e->s_hb, &e->s_q, &e->s_ao, &e->s_ff, &e->s_logits, &e->s_pm, &e->s_pl, &e->s_po, &e->gemm_ws, &e->gemm_ws2, &e->prof_dbytes, &e->d_cross_cnt, &e->d_lnstat,
                    &e->xenc, &e->xscale, &e->xwkt, &e->xwvb, &e->s_qp, &e->s_pu, &e->s_pml, &e->a_logits, &e->a_attn,
                    &e->a_next, &e->a_probs, &e->a_rowsum, &e->a_z, &e->a_mat, &e->a_cost, &e->a_trace, &e->a_pi,
                    &e->a_pj, &e->a_plen, &e->a_meta, &e->a_enc, &e->a_kv, &e->d_tok_lp, &e->d_tok_lp_o, &e->d_fin_lp, &e->d_win_prompt,
                    &e->d_win_slot, &e->d_hyp_out, &e->d_res_tok, &e->d_res_len, &e->d_res_cum, &e->d_res_ns, &e->d_res_lp,
                    &e->d_res_lp_o, &e->d_ev, &e->d_hyp_begin, &e->d_hyp_maxlen, &e->d_win_len, &e->d_win_maxlen,
                    &e->d_sb_off, &e->d_sb_tok, &e->d_sb_val, &e->d_hyp_seed, &e->d_hyp_key, &e->d_win_seed,
                    &e->d_la, &e->d_la_ent})
    b->release();
  for (auto& kv : e->rs_taps) kv.second.pp.release();
  if (e->h_la) (void)hipHostFree(e->h_la);
  if (e->st2) (void)hipStreamDestroy(e->st2);
  if (e->gst) (void)hipStreamDestroy(e->gst);
  if (e->ev_g0) (void)hipEventDestroy(e->ev_g0);
  if (e->ev_g1) (void)hipEventDestroy(e->ev_g1);
  for (hipEvent_t ev : {e->ev_fork, e->ev_mid, e->ev_join})
    if (ev) (void)hipEventDestroy(ev);
  delete e;
}

int wm_set_weight(wm_engine* e, const char* name, const void* d_src, int64_t nbytes, void* stream) {
  return guarded(e, [&] {
    auto it = e->slots.find(name);
    if (it == e->slots.end()) throw std::runtime_error(std::string("wm_set_weight: unknown weight ") + name);
    if ((size_t)nbytes != it->second.bytes)
      throw std::runtime_error(std::string("wm_set_weight: ") + name + " expects " + std::to_string(it->second.bytes) +
                               " bytes, got " + std::to_string(nbytes));
    HIP_OK(hipMemcpyAsync((char*)e->arena.p + it->second.off, d_src, nbytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    it->second.set = true;
    if (it->first == "dec.ckv.w") e->xwkt_ready = false;
  });
}

int32_t wm_weight_count(wm_engine* e) { return e ? (int32_t)e->slot_order.size() : 0; }

int wm_weight_info(wm_engine* e, int32_t i, const char** name, int64_t* nbytes, int32_t* elem_bytes) {
  return guarded(e, [&] {
    if (i < 0 || i >= (int32_t)e->slot_order.size()) throw std::runtime_error("wm_weight_info: index out of range");
    const auto& nm = e->slot_order[i];
    const Slot& s = e->slots.at(nm);
    if (name) *name = nm.c_str();
    if (nbytes) *nbytes = (int64_t)s.bytes;
    if (elem_bytes) *elem_bytes = s.elem;
  });
}

int32_t wm_weights_complete(wm_engine* e) {
  if (!e) return 0;
  for (auto& kv : e->slots)
    if (!kv.second.set) return 0;
  return 1;
}

int wm_logmel(wm_engine* e, const float* d_pcm, int64_t pcm_offset, int64_t n_samples, int64_t frame0, int32_t n_frames,
              float* d_mel, int64_t ld, uint32_t* d_gmax, void* stream) {
  return guarded(e, [&] {
    if (frame0 % 2) throw std::runtime_error("wm_logmel: frame0 must be even (frames are transformed in pairs)");
    const long long n_padded = n_samples + 160;
    ProfScope ps(e, P_LOGMEL, (hipStream_t)stream, 2.0 * 201 * 400 * 2 * n_frames, 4.0 * 160 * n_frames + 4.0 * e->dm.n_mels * n_frames);
    launch_logmel(d_pcm, pcm_offset, n_samples, n_padded, frame0, n_frames, e->fe_window.as<float>(), e->fe_cos.as<float>(),
                  e->fe_sin.as<float>(), e->fe_filt.as<float>(), e->fe_lo.as<int>(), e->fe_hi.as<int>(), e->dm.n_mels,
                  d_mel, ld, d_gmax, (hipStream_t)stream);
  });
}

int wm_logmel_finalize(wm_engine* e, float* d_mel, int64_t n_frames, int64_t ld, const uint32_t* d_gmax, const float* h_gmax,
                       float* h_gmax_out, void* stream) {
  return guarded(e, [&] {
    hipStream_t st = (hipStream_t)stream;
    e->s_pm.ensure(64);
    float* gm = e->s_pm.as<float>();
    if (h_gmax) HIP_OK(hipMemcpyAsync(gm, h_gmax, 4, hipMemcpyHostToDevice, st));
    else launch_ordered_to_float(d_gmax, gm, st);
    if (h_gmax_out) {
      HIP_OK(hipMemcpyAsync(h_gmax_out, gm, 4, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
    }
    launch_logmel_clamp(d_mel, e->dm.n_mels, n_frames, ld, nullptr, gm, st);
    if (h_gmax) HIP_OK(hipStreamSynchronize(st));
  });
}

int wm_encode(wm_engine* e, const float* d_mel, int64_t ld, const int32_t* h_seek, const int32_t* h_nframes, int32_t B,
              void* d_enc_out, void* stream) {
  return guarded(e, [&] {
    require_weights(e);
    check_weights(e);
    hipStream_t st = (hipStream_t)stream;
    const int chunk = std::max(1, e->enc_chunk);
    const size_t per = (size_t)e->dm.n_audio_ctx * e->dm.n_state;
    for (int b0 = 0; b0 < B; b0 += chunk) {
      const int nb = std::min(chunk, B - b0);
      for (int i = 0; i < nb; ++i)
        if (h_nframes[b0 + i] < 0 || h_nframes[b0 + i] > 3000 || h_seek[b0 + i] < 0 || h_seek[b0 + i] + h_nframes[b0 + i] > ld)
          throw std::runtime_error("wm_encode: window outside the mel buffer");
      encode_chunk(e, d_mel, ld, h_seek + b0, h_nframes + b0, nb, (bf16*)d_enc_out + (size_t)b0 * per, st);
      HIP_OK(hipStreamSynchronize(st));   // seek/len staging buffers are reused by the next chunk
    }
  });
}

int wm_reserve(wm_engine* e, int32_t n_slots, int32_t n_hyp, void* stream) {
  return guarded(e, [&] {
    (void)stream;
    reserve(e, n_slots, n_hyp);
  });
}

int wm_cross_kv(wm_engine* e, const void* d_enc, int32_t B, int32_t slot0, void* stream) {
  return guarded(e, [&] {
    require_weights(e);
    check_weights(e);
    if (slot0 < 0 || slot0 + B > e->n_slots) throw std::runtime_error("wm_cross_kv: slots out of range (wm_reserve first)");
    const auto& m = e->dm;
    const int d = m.n_state, T = m.n_audio_ctx;
    if (e->cross_mode == 1 && e->cross_fp8) {   // factored, fp8: e4m3 image + per-position scales
      const size_t per = (size_t)T * d;
      ProfScope ps(e, P_CROSSKV_GEMM, (hipStream_t)stream, 0, 3.0 * B * per + 4.0 * B * T);
      launch_xquant8((const bf16*)d_enc, (long long)B * T, d, e->xenc.as<unsigned char>() + (size_t)slot0 * per,
                     e->xscale.as<float>() + (size_t)slot0 * T, (hipStream_t)stream);
      return;
    }
    if (e->cross_mode == 1) {   // factored: the slot holds the encoder output itself, tile-blocked
      const size_t per = (size_t)T * d;
      ProfScope ps(e, P_CROSSKV_GEMM, (hipStream_t)stream, 0, 2.0 * 2 * B * per);
      launch_xblock((const bf16*)d_enc, B, T, d, e->xenc.as<bf16>() + (size_t)slot0 * xblock_slot_elems(T, d), true,
                    (hipStream_t)stream);
      return;
    }
    if (e->cross_kv_fp8) {
      // fp8 panels (1) / their dequantised reference form (2): the same GEMM projects KV8_STAGE_WINDOWS windows at a
      // time into the bf16 staging buffer in the panel layout, the quantiser writes that chunk's slots
      hipStream_t st = (hipStream_t)stream;
      const int H = m.n_head, L = m.n_dec_layer;
      const long long win_rows = (long long)H * T;                       // 64-value rows per (layer, k|v, window)
      constexpr int CW = wm_engine::KV8_STAGE_WINDOWS;
      // (sized to this call's chunk: a one-window call, the sequential transcribe, stages one window)
      e->kv8_stage.ensure((size_t)L * 2 * std::min(CW, (int)B) * win_rows * 64 * 2);
      for (int b0 = 0; b0 < B; b0 += CW) {
        const int nb = std::min(CW, B - b0);
        GemmEpi ep = epi_of(EPI_CROSS_KV, e->kv8_stage.p, 0, e->Wf("dec.ckv.b"));
        ep.rpb = T; ep.d = d; ep.head_dim = 64; ep.n_head = H; ep.n_slots = nb; ep.slot0 = 0;
        gemm_p(e, P_CROSSKV_GEMM, amat((const bf16*)d_enc + (size_t)b0 * T * d, d), e->Wb("dec.ckv.w"), d, nb * T, L * 2 * d,
               d, ep, st);
        const long long n_rows = (long long)L * 2 * nb * win_rows;
        ProfScope ps(e, P_CROSSKV_GEMM, st, 0, (e->cross_kv_fp8 == 1 ? 193.0 : 256.0) * n_rows);
        launch_kv8_quant(e->kv8_stage.as<bf16>(), n_rows, nb * win_rows, (long long)e->n_slots * win_rows,
                         (long long)(slot0 + b0) * win_rows, e->ckv.as<unsigned char>(), e->ckv_exp.as<unsigned char>(),
                         e->cross_kv_fp8 == 2 ? e->ckv.as<bf16>() : nullptr, st);
      }
      return;
    }
    GemmEpi ep = epi_of(EPI_CROSS_KV, e->ckv.p, 0, e->Wf("dec.ckv.b"));
    ep.rpb = T; ep.d = d; ep.head_dim = 64; ep.n_head = m.n_head; ep.n_slots = e->n_slots; ep.slot0 = slot0;
    gemm_p(e, P_CROSSKV_GEMM, amat((const bf16*)d_enc, d), e->Wb("dec.ckv.w"), d, B * T, m.n_dec_layer * 2 * d, d, ep,
           (hipStream_t)stream);
  });
}

int wm_generate(wm_engine* e, const wm_generate_args* a, void* stream) {
  return guarded(e, [&] {
    require_weights(e);
    generate(e, a, (hipStream_t)stream);
  });
}

int wm_generate_seeded(wm_engine* e, const wm_generate_args* a, const uint64_t* h_seeds, void* stream) {
  return guarded(e, [&] {
    require_weights(e);
    struct SeedScope {                    // the seeds belong to this call alone, exceptions included
      wm_engine* e;
      SeedScope(wm_engine* e_, const uint64_t* s) : e(e_) { e->call_seeds = s; }
      ~SeedScope() { e->call_seeds = nullptr; }
    } scope(e, a->temperature > 0.f ? h_seeds : nullptr);
    generate(e, a, (hipStream_t)stream);
  });
}

int wm_generate_multilingual(wm_engine* e, const wm_generate_args* a, const wm_language_auto* la, const uint64_t* h_seeds,
                             void* stream) {
  if (!la) return wm_generate_seeded(e, a, h_seeds, stream);
  return guarded(e, [&] {
    require_weights(e);
    const std::string who = "wm_generate_multilingual: ";
    const int n_langs = la->n_langs, lang_begin = la->lang_begin;
    if (n_langs <= 0 || n_langs > SEARCH_LANG_MAX)
      throw std::runtime_error(who + "n_langs outside 1.." + std::to_string(SEARCH_LANG_MAX));
    if (lang_begin < 0 || lang_begin + n_langs > e->dm.n_vocab)
      throw std::runtime_error(who + "lang_begin .. lang_begin + n_langs outside the vocabulary");
    if (la->h_allowed && std::none_of(la->h_allowed, la->h_allowed + n_langs, [](uint8_t v) { return v != 0; }))
      throw std::runtime_error(who + "h_allowed sets no language");
    const int W = a->n_windows;
    if (W <= 0) return;
    if (!la->h_lang_pos || !la->h_lang || !la->h_lang_prob) throw std::runtime_error(who + "null argument");
    const WinArgs wa = window_args(e, a);
    LangCall lc;
    lc.lang_begin = lang_begin; lc.n_langs = n_langs;
    lc.pos.assign(W, -1); lc.aidx.assign(W, -1);
    std::vector<int> slots;                                  // the auto windows' slots, in call order
    for (int w = 0; w < W; ++w) {
      const int pos = la->h_lang_pos[w];
      if (pos < 0) continue;
      const std::string ww = who + "window " + std::to_string(w) + ": ";
      if (pos >= wa.len[w])
        throw std::runtime_error(ww + "language position " + std::to_string(pos) + " outside its prompt of " +
                                 std::to_string(wa.len[w]) + " tokens");
      const int* pr = a->h_prompts + (size_t)w * a->prompt_len;
      if (pr[pos] < lang_begin || pr[pos] >= lang_begin + n_langs)
        throw std::runtime_error(ww + "token " + std::to_string(pr[pos]) + " at language position " + std::to_string(pos) +
                                 " is not a language token");
      if (pos == 0 || pr[pos - 1] != e->dm.sot)
        throw std::runtime_error(ww + "the token before language position " + std::to_string(pos) +
                                 " is not <|startoftranscript|>");
      if (a->h_slots[w] < 0 || a->h_slots[w] >= e->n_slots) throw std::runtime_error(ww + "slot outside the reserved slots");
      lc.pos[w] = pos; lc.aidx[w] = (int)slots.size();
      slots.push_back(a->h_slots[w]);
    }
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)slots.size(), d = e->dm.n_state;
    std::vector<std::vector<int>> keep;                      // the detection passes' uploads (no wait of their own)
    int* err = nullptr;
    float* d_probs = nullptr;
    if (n > 0) {
      // wm_language_id over the auto windows: the same passes (160 rows each, in call order), the same head, but the
      // results stay on the device and nothing waits for them.  Hypothesis capacity for a pass is reserved here, once:
      // generate()'s own reserve then grows the tables or leaves them, before it takes any pointer into them, and the
      // self-KV the passes write (position 0 of their rows) is overwritten by the prefill before anything reads it.
      constexpr int PASS = 160;
      reserve(e, e->n_slots, std::min(n, PASS));
      e->d_la.ensure((4 + (size_t)n * (2 + n_langs)) * 4);
      e->a_meta.ensure((size_t)SEARCH_LANG_MAX);
      err = e->d_la.as<int>() + 1;                           // (an error word of its own: generate() clears the decode's)
      int* d_top = e->d_la.as<int>() + 4;
      float* d_top_prob = (float*)(d_top + n);
      d_probs = d_top_prob + n;
      HIP_OK(hipMemsetAsync(e->d_la.p, 0, 4 * 4, st));
      if (la->h_allowed) HIP_OK(hipMemcpyAsync(e->a_meta.p, la->h_allowed, n_langs, hipMemcpyHostToDevice, st));
      const std::vector<int> toks(std::min(n, PASS), e->dm.sot);
      for (int r0 = 0; r0 < n; r0 += PASS) {
        const int nr = std::min(PASS, n - r0);
        forward(e, nr, slots.data() + r0, 1, toks.data(), nullptr, 1, nullptr, 0, nullptr, st, nullptr, true, &keep);
        launch_lang_head(e->s_x.as<float>(), d, nr, d, e->Wf("dec.ln.w"), e->Wf("dec.ln.b"), e->Wb("dec.embed"), lang_begin,
                         n_langs, la->h_allowed ? e->a_meta.as<unsigned char>() : nullptr, d_probs + (size_t)r0 * n_langs,
                         d_top + r0, d_top_prob + r0, r0, err, st);
      }
      lc.d_top = d_top;
      // the results' way back: queued here, delivered by generate()'s own final synchronise (no wait of its own)
      const size_t nb = (4 + (size_t)n * (2 + n_langs)) * 4;
      if (nb > e->h_la_bytes) {
        if (e->h_la) HIP_OK(hipHostFree(e->h_la));
        e->h_la = nullptr;
        e->h_la_bytes = 0;
        HIP_OK(hipHostMalloc(&e->h_la, nb, hipHostMallocDefault));
        e->h_la_bytes = nb;
      }
      HIP_OK(hipMemcpyAsync(e->h_la, e->d_la.p, nb, hipMemcpyDeviceToHost, st));
    }
    struct Scope {                        // the seeds and the language state belong to this call alone
      wm_engine* e;
      Scope(wm_engine* e_, const uint64_t* s, LangCall* l) : e(e_) { e->call_seeds = s; e->call_lang = l; }
      ~Scope() { e->call_seeds = nullptr; e->call_lang = nullptr; }
    } scope(e, a->temperature > 0.f ? h_seeds : nullptr, n > 0 ? &lc : nullptr);
    try {
      generate(e, a, st);
    } catch (...) {
      (void)hipStreamSynchronize(st);     // (`keep` and `slots` outlive whatever the stream still holds)
      throw;
    }
    // generate() has synchronised the stream for its own results: the language results' copy, queued before it, is in
    std::vector<float> host((size_t)n * (2 + n_langs) + 4, 0.f);
    if (n > 0) std::memcpy(host.data(), e->h_la, host.size() * 4);
    const int* h_top = (const int*)host.data() + 4;
    const float* h_top_prob = host.data() + 4 + n;
    const float* h_pr = h_top_prob + n;
    int failed = -1;
    for (int w = 0; w < W; ++w) {
      const int i = lc.aidx[w];
      la->h_lang[w] = i >= 0 ? h_top[i] : -1;
      la->h_lang_prob[w] = i >= 0 ? h_top_prob[i] : 0.f;
      if (la->h_probs) {
        float* dst = la->h_probs + (size_t)w * n_langs;
        if (i >= 0) std::memcpy(dst, h_pr + (size_t)i * n_langs, (size_t)n_langs * 4);
        else std::fill(dst, dst + n_langs, 0.f);
      }
      if (i >= 0 && h_top[i] < 0 && failed < 0) failed = w;
    }
    if (failed >= 0)
      throw std::runtime_error(who + "non-finite language logits, window " + std::to_string(failed) +
                               " (row " + std::to_string(((const int*)host.data())[2]) + ")");
  });
}

int wm_forward(wm_engine* e, int32_t n_seq, const int32_t* h_slots, int32_t seq_len, const int32_t* h_tokens, float* d_logits,
               int32_t last_only, const int32_t* h_align_heads, int32_t n_align, float* d_attn, void* stream) {
  return guarded(e, [&] {
    require_weights(e);
    forward(e, n_seq, h_slots, seq_len, h_tokens, d_logits, last_only, h_align_heads, n_align, d_attn, (hipStream_t)stream);
  });
}

int wm_detect_language(wm_engine* e, int32_t n, const int32_t* h_slots, int32_t lang_begin, int32_t n_langs,
                       float* h_probs, void* stream) {
  return guarded(e, [&] {
    require_weights(e);
    if (n <= 0) return;
    if (lang_begin < 0 || n_langs <= 0 || lang_begin + n_langs > e->dm.n_vocab)
      throw std::runtime_error("wm_detect_language: language tokens outside the vocabulary");
    hipStream_t st = (hipStream_t)stream;
    const int V = e->dm.n_vocab;
    std::vector<int> toks(n, e->dm.sot);
    e->a_logits.ensure((size_t)n * V * 4);
    forward(e, n, h_slots, 1, toks.data(), e->a_logits.as<float>(), 1, nullptr, 0, nullptr, st);
    e->a_probs.ensure((size_t)n * n_langs * 4);
    launch_lang_probs(e->a_logits.as<float>(), V, n, lang_begin, n_langs, e->a_probs.as<float>(), st);
    HIP_OK(hipMemcpyAsync(h_probs, e->a_probs.p, (size_t)n * n_langs * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  });
}

int wm_language_id(wm_engine* e, int32_t n, const int32_t* h_slots, int32_t lang_begin, int32_t n_langs,
                   const uint8_t* h_allowed, float* h_probs, int32_t* h_top, float* h_top_prob, void* stream) {
  return guarded(e, [&] {
    require_weights(e);
    if (n < 0) throw std::runtime_error("wm_language_id: n must be >= 0");
    if (n_langs <= 0 || n_langs > SEARCH_LANG_MAX)
      throw std::runtime_error("wm_language_id: n_langs outside 1.." + std::to_string(SEARCH_LANG_MAX));
    if (lang_begin < 0 || lang_begin + n_langs > e->dm.n_vocab)
      throw std::runtime_error("wm_language_id: lang_begin .. lang_begin + n_langs outside the vocabulary");
    if (h_allowed && std::none_of(h_allowed, h_allowed + n_langs, [](uint8_t v) { return v != 0; }))
      throw std::runtime_error("wm_language_id: h_allowed sets no language");
    if (n == 0) return;
    if (!h_slots || !h_probs || !h_top || !h_top_prob) throw std::runtime_error("wm_language_id: null argument");
    for (int i = 0; i < n; ++i)
      if (h_slots[i] < 0 || h_slots[i] >= e->n_slots)
        throw std::runtime_error("wm_language_id: h_slots[" + std::to_string(i) + "] outside the reserved slots");
    hipStream_t st = (hipStream_t)stream;
    const int d = e->dm.n_state;
    // rows per decoder pass (the hypothesis tables and the step scratch grow to one pass, not to n)
    constexpr int PASS = 160;
    const int cap = std::min(n, PASS);
    // a pass's results packed in one buffer, [rows][n_langs] probabilities, [rows] best index, [rows] its probability:
    // one copy back per pass
    const size_t per_row = (size_t)n_langs + 2;
    e->a_probs.ensure((size_t)cap * per_row * 4);
    e->a_meta.ensure((size_t)SEARCH_LANG_MAX);
    reserve(e, e->n_slots, cap);                             // (also the error word's buffer)
    int* err = e->d_n_active.as<int>() + 1;
    HIP_OK(hipMemsetAsync(err, 0, 3 * 4, st));
    if (h_allowed) HIP_OK(hipMemcpyAsync(e->a_meta.p, h_allowed, n_langs, hipMemcpyHostToDevice, st));
    const std::vector<int> toks(cap, e->dm.sot);
    std::vector<float> host((size_t)n * per_row);
    for (int r0 = 0; r0 < n; r0 += PASS) {
      const int nr = std::min(PASS, n - r0);
      forward(e, nr, h_slots + r0, 1, toks.data(), nullptr, 1, nullptr, 0, nullptr, st, nullptr, true);
      float* d_probs = e->a_probs.as<float>();
      int* d_top = (int*)(d_probs + (size_t)nr * n_langs);
      float* d_top_prob = d_probs + (size_t)nr * n_langs + nr;
      launch_lang_head(e->s_x.as<float>(), d, nr, d, e->Wf("dec.ln.w"), e->Wf("dec.ln.b"), e->Wb("dec.embed"), lang_begin,
                       n_langs, h_allowed ? e->a_meta.as<unsigned char>() : nullptr, d_probs, d_top, d_top_prob, r0, err, st);
      HIP_OK(hipMemcpyAsync(host.data() + (size_t)r0 * per_row, d_probs, (size_t)nr * per_row * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));                        // (a later pass reuses a_probs: each copy is ordered before it)
    bool failed = false;
    for (int r0 = 0; r0 < n; r0 += PASS) {
      const int nr = std::min(PASS, n - r0);
      const float* src = host.data() + (size_t)r0 * per_row;
      std::memcpy(h_probs + (size_t)r0 * n_langs, src, (size_t)nr * n_langs * 4);
      std::memcpy(h_top + r0, src + (size_t)nr * n_langs, (size_t)nr * 4);
      std::memcpy(h_top_prob + r0, src + (size_t)nr * n_langs + nr, (size_t)nr * 4);
      for (int i = 0; i < nr; ++i) failed |= h_top[r0 + i] < 0;
    }
    if (failed) {                                            // a failed row has no best language; the error word names one
      int h_err[3] = {0, 0, 0};
      HIP_OK(hipMemcpyAsync(h_err, err, sizeof(h_err), hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      throw std::runtime_error("wm_language_id: non-finite logits, row " + std::to_string(h_err[1]));
    }
  });
}

int64_t wm_device_bytes(wm_engine* e) { return e ? (int64_t)e->device_bytes() : 0; }

int wm_frame_energy(wm_engine* e, const float* d_pcm, int64_t n_samples, int32_t frame, float* d_db, void* stream) {
  return guarded(e, [&] {
    if (frame <= 0) throw std::runtime_error("wm_frame_energy: bad frame size");
    const int frames = (int)((n_samples + frame - 1) / frame);
    launch_frame_energy(d_pcm, n_samples, frame, frames, d_db, (hipStream_t)stream);
  });
}

int wm_pcm_from_s16(wm_engine* e, const int16_t* d_src, int64_t n, float* d_dst, void* stream) {
  return guarded(e, [&] {
    if (n < 0) throw std::runtime_error("wm_pcm_from_s16: negative length");
    launch_pcm_s16((const short*)d_src, n, d_dst, (hipStream_t)stream);
  });
}

int wm_resample_plan(int32_t src_rate, int32_t* up, int32_t* down, int32_t* half_len) {
  try {
    const RsPlan p = rs_plan(src_rate, "wm_resample_plan");
    if (up) *up = p.up;
    if (down) *down = p.down;
    if (half_len) *half_len = p.half;
    return 0;
  } catch (const std::exception& ex) {
    g_err = ex.what();
    return -1;
  }
}

int wm_resample_taps(int32_t src_rate, float* h_taps) {
  try {
    if (!h_taps) throw std::runtime_error("wm_resample_taps: null argument");
    const std::vector<double> h = rs_taps_f64(rs_plan(src_rate, "wm_resample_taps"));
    for (size_t k = 0; k < h.size(); ++k) h_taps[k] = (float)h[k];
    return 0;
  } catch (const std::exception& ex) {
    g_err = ex.what();
    return -1;
  }
}

int wm_resample(wm_engine* e, const void* d_src, int32_t fmt, int32_t channels, int32_t channel, int32_t src_rate,
                int64_t src_offset, int64_t n_src, int64_t n_total, int64_t out0, int64_t n_out, float* d_dst,
                void* stream) {
  return guarded(e, [&] {
    const RsPlan p = rs_plan(src_rate, "wm_resample");
    auto S = [](long long v) { return std::to_string(v); };
    if (fmt != 0 && fmt != 1) throw std::runtime_error("wm_resample: fmt " + S(fmt) + " (0 = s16, 1 = f32)");
    if (channels < 1 || channels > 8) throw std::runtime_error("wm_resample: channels " + S(channels) + " (1 .. 8)");
    if (channel < -1 || channel >= channels)
      throw std::runtime_error("wm_resample: channel " + S(channel) + " of " + S(channels) + " (-1 = mean of all)");
    if (src_offset < 0 || n_src < 0 || out0 < 0 || n_out < 0 || n_total < -1)
      throw std::runtime_error("wm_resample: negative offset or length");
    if (n_total >= 0 && src_offset + n_src > n_total)
      throw std::runtime_error("wm_resample: source span [" + S(src_offset) + ", " + S(src_offset + n_src) +
                               ") past the end of the file (" + S(n_total) + " frames)");
    if (n_total >= 0 && out0 + n_out > ceil_div(n_total * p.up, p.down))
      throw std::runtime_error("wm_resample: outputs [" + S(out0) + ", " + S(out0 + n_out) + ") past the end of the output (" +
                               S(ceil_div(n_total * p.up, p.down)) + " samples)");
    if (n_out == 0) return;
    if (!d_dst || (!d_src && n_src > 0)) throw std::runtime_error("wm_resample: null buffer");
    // frames the outputs read, clipped to the file: all of them must be in the span given
    const long long lo = std::max(0LL, ceil_div(out0 * p.down - p.half, p.up));
    long long hi = ((out0 + n_out - 1) * p.down + p.half) / p.up;
    if (n_total >= 0) hi = std::min<long long>(hi, n_total - 1);
    if (hi >= lo && (lo < src_offset || hi >= src_offset + n_src))
      throw std::runtime_error("wm_resample: outputs [" + S(out0) + ", " + S(out0 + n_out) + ") need source frames [" +
                               S(lo) + ", " + S(hi) + "], missing from the span given [" + S(src_offset) + ", " +
                               S(src_offset + n_src) + ")");
    int T = 0;
    const float* pp = rs_device_taps(e, p, &T);
    launch_resample(d_src, fmt, channels, channel, src_offset, n_src, n_total, pp, p.up, p.down, p.half, T, out0, n_out,
                    d_dst, (hipStream_t)stream);
  });
}

int wm_cross_fp8_quantize(wm_engine* e, const void* d_enc, int64_t rows, uint8_t* d_codes, float* d_scale, void* stream) {
  return guarded(e, [&] {
    launch_xquant8((const bf16*)d_enc, rows, e->dm.n_state, d_codes, d_scale, (hipStream_t)stream);
  });
}

int wm_cross_kv_fp8_quantize(wm_engine* e, const void* d_rows_bf16, int64_t n_rows, uint8_t* d_codes, uint8_t* d_exp,
                             void* stream) {
  return guarded(e, [&] {
    if (n_rows < 0) throw std::runtime_error("wm_cross_kv_fp8_quantize: negative row count");
    if (n_rows == 0) return;
    if (!d_rows_bf16 || !d_codes || !d_exp) throw std::runtime_error("wm_cross_kv_fp8_quantize: null buffer");
    launch_kv8_quant((const bf16*)d_rows_bf16, n_rows, n_rows, n_rows, 0, d_codes, d_exp, nullptr, (hipStream_t)stream);
  });
}

int wm_vad_probs(wm_engine* e, const wm_vad_weights* w, const float* d_pcm, int64_t n_samples, float* d_work,
                 float* d_probs, void* stream) {
  return guarded(e, [&] {
    if (!w || !w->stft_basis || !w->w_ih || !w->w_hh || !w->b_ih || !w->b_hh || !w->head_w || !w->head_b)
      throw std::runtime_error("wm_vad_probs: missing weight");
    if (n_samples < 0 || n_samples % 512) throw std::runtime_error("wm_vad_probs: n_samples must be a multiple of 512");
    VadW vw;
    vw.basis = w->stft_basis;
    for (int i = 0; i < 4; ++i) {
      if (!w->conv_w[i] || !w->conv_b[i]) throw std::runtime_error("wm_vad_probs: missing conv weight");
      vw.cw[i] = w->conv_w[i];
      vw.cb[i] = w->conv_b[i];
    }
    vw.w_ih = w->w_ih; vw.w_hh = w->w_hh; vw.b_ih = w->b_ih; vw.b_hh = w->b_hh;
    vw.dec_w = w->head_w; vw.dec_b = w->head_b;
    launch_vad(vw, d_pcm, n_samples / 512, d_work, d_probs, (hipStream_t)stream);
  });
}

int wm_align(wm_engine* e, int32_t slot, int32_t sot_len, const int32_t* h_sot, int32_t n_text, const int32_t* h_text,
             int32_t num_frames, const int32_t* h_heads, int32_t n_heads, int32_t median_filter_width, float* h_probs,
             int32_t* h_text_idx, int32_t* h_time_idx, int32_t* h_path_len, void* stream) {
  return guarded(e, [&] {
    require_weights(e);
    check_weights(e);
    align(e, slot, sot_len, h_sot, n_text, h_text, num_frames, h_heads, n_heads, median_filter_width, h_probs, h_text_idx,
          h_time_idx, h_path_len, (hipStream_t)stream);
  });
}

int wm_align_batch(wm_engine* e, int32_t n, const int32_t* h_slots, int32_t sot_len, const int32_t* h_sot,
                   const int32_t* h_text_off, const int32_t* h_text, const int32_t* h_num_frames, const int32_t* h_heads,
                   int32_t n_heads, int32_t median_filter_width, float* h_probs, const int64_t* h_path_off,
                   int32_t* h_text_idx, int32_t* h_time_idx, int32_t* h_path_len, void* stream) {
  return guarded(e, [&] {
    require_weights(e);
    check_weights(e);
    for (int i = 0; i < n; ++i)
      if (h_slots[i] < 0 || h_slots[i] >= e->n_slots) throw std::runtime_error("wm_align_batch: slot out of range");
    align_batch(e, n, h_slots, sot_len, h_sot, h_text_off, h_text, h_num_frames, h_heads, n_heads, median_filter_width,
                h_probs, (const long long*)h_path_off, h_text_idx, h_time_idx, h_path_len, (hipStream_t)stream);
  });
}

int wm_dtw(wm_engine* e, const float* d_cost, int32_t n, int32_t m, int32_t* h_text_idx, int32_t* h_time_idx,
           int32_t* h_path_len, void* stream) {
  return guarded(e, [&] { dtw_run(e, d_cost, n, m, h_text_idx, h_time_idx, h_path_len, (hipStream_t)stream); });
}

int wm_dtw_open(wm_engine* e, const float* d_cost, int32_t n, int32_t m, int32_t* h_text_idx, int32_t* h_time_idx,
                int32_t* h_path_len, int32_t* h_rows, void* stream) {
  return guarded(e, [&] {
    if (!h_rows) throw std::runtime_error("wm_dtw_open: null h_rows");
    dtw_run(e, d_cost, n, m, h_text_idx, h_time_idx, h_path_len, (hipStream_t)stream, h_rows);
  });
}

int wm_set_sequence_bias(wm_engine* e, int32_t n, const int32_t* h_off, const int32_t* h_tokens, const float* h_bias,
                         void* stream) {
  return guarded(e, [&] {
    const std::string who = "wm_set_sequence_bias: ";
    if (n < 0 || n > SEARCH_BIAS_MAX)
      throw std::runtime_error(who + "n must be in [0, " + std::to_string(SEARCH_BIAS_MAX) + "]");
    if (n == 0) {
      e->n_seq_bias = 0;
      return;
    }
    if (!h_off || !h_tokens || !h_bias) throw std::runtime_error(who + "null table");
    // everything is validated before the engine's table is touched: a refused call leaves the previous one in place
    if (h_off[0] != 0) throw std::runtime_error(who + "offsets must start at 0");
    for (int j = 0; j < n; ++j) {
      const std::string ent = "entry " + std::to_string(j);
      const long long nj = (long long)h_off[j + 1] - h_off[j];
      if (nj < 1 || nj > SEARCH_BIAS_LEN)
        throw std::runtime_error(who + ent + " has " + std::to_string(nj) + " tokens (offsets must ascend by 1 .. " +
                                 std::to_string(SEARCH_BIAS_LEN) + ")");
      for (int i = h_off[j]; i < h_off[j + 1]; ++i)
        if (h_tokens[i] < 0 || h_tokens[i] >= e->dm.n_vocab)
          throw std::runtime_error(who + ent + " holds token " + std::to_string(h_tokens[i]) + " outside the vocabulary");
      if (!std::isfinite(h_bias[j])) throw std::runtime_error(who + ent + " has a non-finite bias");
    }
    // device order: by completing id, entries of one id in the caller's order (search.hip header)
    std::vector<int> order(n);
    for (int j = 0; j < n; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return h_tokens[h_off[a + 1] - 1] < h_tokens[h_off[b + 1] - 1]; });
    std::vector<int> off(n + 1, 0), tok;
    std::vector<float> val(n);
    tok.reserve(h_off[n]);
    for (int r = 0; r < n; ++r) {
      const int j = order[r];
      tok.insert(tok.end(), h_tokens + h_off[j], h_tokens + h_off[j + 1]);
      off[r + 1] = (int)tok.size();
      val[r] = h_bias[j];
    }
    hipStream_t st = (hipStream_t)stream;
    e->d_sb_off.ensure((size_t)(SEARCH_BIAS_MAX + 1) * 4);
    e->d_sb_tok.ensure((size_t)SEARCH_BIAS_MAX * SEARCH_BIAS_LEN * 4);
    e->d_sb_val.ensure((size_t)SEARCH_BIAS_MAX * 4);
    e->n_seq_bias = 0;            // (a failed copy leaves no half-written table in use)
    HIP_OK(hipMemcpyAsync(e->d_sb_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(e->d_sb_tok.p, tok.data(), tok.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(e->d_sb_val.p, val.data(), val.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));        // the host images above end with this call
    e->n_seq_bias = n;
  });
}

int wm_align_open_batch(wm_engine* e, int32_t n, const int32_t* h_slots, int32_t sot_len, const int32_t* h_sot,
                        const int32_t* h_text_off, const int32_t* h_text, const int32_t* h_num_frames,
                        const int32_t* h_heads, int32_t n_heads, int32_t median_filter_width, float* h_probs,
                        const int64_t* h_path_off, int32_t* h_text_idx, int32_t* h_time_idx, int32_t* h_path_len,
                        int32_t* h_rows, void* stream) {
  return guarded(e, [&] {
    require_weights(e);
    check_weights(e);
    if (!h_rows) throw std::runtime_error("wm_align_open_batch: null h_rows");
    for (int i = 0; i < n; ++i)
      if (h_slots[i] < 0 || h_slots[i] >= e->n_slots) throw std::runtime_error("wm_align_open_batch: slot out of range");
    align_batch(e, n, h_slots, sot_len, h_sot, h_text_off, h_text, h_num_frames, h_heads, n_heads, median_filter_width,
                h_probs, (const long long*)h_path_off, h_text_idx, h_time_idx, h_path_len, (hipStream_t)stream, h_rows);
  });
}

int wm_encoder_attention(wm_engine* e, const void* d_qkv, void* d_out, int32_t B, int32_t T, void* stream) {
  return guarded(e, [&] {
    if (B <= 0 || T <= 0) throw std::runtime_error("wm_encoder_attention: bad B/T");
    launch_attn_enc((const bf16*)d_qkv, (bf16*)d_out, B, T, e->dm.n_state, e->dm.n_head, (hipStream_t)stream);
  });
}

int wm_set_option(wm_engine* e, const char* key, int64_t value) {
  return guarded(e, [&] {
    if (!key) throw std::runtime_error("wm_set_option: null key");
    const std::string k(key);
    bool cols = false;
    if (const OptRow* r = find_option(k)) {
      r->set(e, value);
    } else if (int* p = dec_proj_option(e, k, "wm_set_option", &cols)) {
      if (cols && value != 32 && value != 64) throw std::runtime_error("wm_set_option: decode_gemm_cols.<proj> is 32 or 64");
      if (!cols && (value < -2 || value > 160)) throw std::runtime_error("wm_set_option: decode_gemm.<proj> in [-2, 160]");
      *p = (int)value;
    } else {
      throw std::runtime_error("wm_set_option: unknown option " + k);
    }
  });
}

int wm_get_option(wm_engine* e, const char* key, int64_t* value) {
  return guarded(e, [&] {
    if (!key || !value) throw std::runtime_error("wm_get_option: null argument");
    const std::string k(key);
    bool cols = false;
    if (const OptRow* r = find_option(k)) *value = r->get(e);
    else if (const int* p = dec_proj_option(e, k, "wm_get_option", &cols)) *value = *p;
    else throw std::runtime_error("wm_get_option: unknown option " + k);
  });
}

int32_t wm_profile_classes(void) { return P_N; }
const char* wm_profile_name(int32_t cls) { return (cls >= 0 && cls < P_N) ? kProfNames[cls] : ""; }

int wm_profile_select(wm_engine* e, uint32_t class_mask) {
  return guarded(e, [&] {
    HIP_OK(hipDeviceSynchronize());
    if (!class_mask) {        // stop recording; keep what was recorded for wm_profile_read
      e->prof_on = false;
      return;
    }
    for (int c = 0; c < P_N; ++c) {
      for (auto& pr : e->prof_ev[c]) { e->ev_pool.push_back(pr.first); e->ev_pool.push_back(pr.second); }
      e->prof_ev[c].clear();
      e->prof_flops[c] = 0;
      e->prof_bytes[c] = 0;
    }
    e->prof_dbytes.ensure((size_t)P_N * STAT_SLOTS * sizeof(unsigned long long));
    HIP_OK(hipMemset(e->prof_dbytes.p, 0, (size_t)P_N * STAT_SLOTS * sizeof(unsigned long long)));
    e->prof_mask = class_mask;
    e->prof_on = true;
  });
}

int wm_profile(wm_engine* e, int32_t enable) { return wm_profile_select(e, enable ? ((1u << P_N) - 1u) : 0u); }

int wm_profile_read(wm_engine* e, int32_t cls, int64_t* launches, double* ms, double* flops, double* bytes) {
  return guarded(e, [&] {
    if (cls < 0 || cls >= P_N) throw std::runtime_error("wm_profile_read: bad class");
    HIP_OK(hipDeviceSynchronize());
    double t = 0;
    for (auto& pr : e->prof_ev[cls]) {
      float x = 0;
      HIP_OK(hipEventElapsedTime(&x, pr.first, pr.second));
      t += x;
    }
    std::vector<unsigned long long> slots(STAT_SLOTS, 0);
    if (e->prof_dbytes.p)
      HIP_OK(hipMemcpy(slots.data(), e->prof_dbytes.as<unsigned long long>() + (size_t)cls * STAT_SLOTS,
                       STAT_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double dbytes = 0;
    for (auto v : slots) dbytes += (double)v;
    *launches = (int64_t)e->prof_ev[cls].size();
    *ms = t;
    *flops = e->prof_flops[cls];
    *bytes = e->prof_bytes[cls] + dbytes;
  });
}

}  // extern "C"
