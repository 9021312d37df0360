#pragma once
#include "common.h"

#define SEARCH_SB 1024           // threads per logits row (logits_select_kernel)
#define SEARCH_PER 52            // ids per thread: vocab <= SEARCH_SB * SEARCH_PER = 53248
#define SEARCH_BIAS_MAX 1024     // sequence-bias table: entries
#define SEARCH_BIAS_LEN 16       // ... and tokens per entry
#define SEARCH_LANG_MAX 128      // language head: languages per call (Whisper has 99 or 100)

struct SearchParams {
  const float* logits;   // [rows][V] f32, row r belongs to hypothesis r
  long long ldl;
  int V;
  int* tokens;           // [n_hyp][n_ctx] full sequences (prompt + generated)
  int n_ctx;
  int* seq_len;          // [n_hyp]
  int sample_begin;      // prompt length
  // suppressed ids as per-thread bit words: bit k of word t <=> id t + k * SEARCH_SB is suppressed (or >= V); one
  // 8-B load per thread instead of one dependent byte load per element (search_suppress_bits builds it)
  const unsigned long long* suppress_bits;   // [SEARCH_SB]
  int suppress_blank, blank, eot, no_timestamps, ts_begin, max_initial;   // max_initial < 0: none
  int with_ts;
  int* done;             // [n_hyp]
  int mode;              // 0 greedy, 1 beam candidates, 2 sampling
  int topk;              // beam: beam_size + 1
  float inv_temperature;
  unsigned long long seed;
  int step;
  int max_length;
  int abl;               // diagnostics (VLOG_AMD_SEL_ABL): bit 1 = beam top-k by K rounds over the row
  // greedy / sampling state (updated in place)
  float* cum;            // [n_hyp]
  int* row_tok; int* row_pos;      // next step's decoder input per hypothesis
  int* n_active;         // decremented when a hypothesis finishes
  // beam outputs
  int* cand_tok; float* cand_lp;   // [n_hyp][topk]
  // compacted row set (nullptr: row r is hypothesis r): block r reads logits row r and decodes hypothesis
  // row_hyp[r]; row_tok / row_pos are written per ROW (the next pass's inputs), the rest per hypothesis
  const int* row_hyp;
  // device error word (nullptr: none): [0] code (1 non-finite logits row, 2 no legal token), [1] hypothesis,
  // [2] tokens sampled before the failing step; the first failure wins (wm_report_error)
  int* err;
  // optional per-step records [n_hyp][n_ctx] (nullptr: off): log-prob of the token chosen at sequence position
  // len (the final <|endoftext|> included) and, greedy / sampling, the best log-prob among the other allowed tokens
  float* tok_lp;
  float* tok_lp_other;
  // results of finished hypotheses by OUTPUT id (greedy / sampling: the row-set decode, whose hypothesis slots are
  // reused; nullptr: the host reads the hypothesis tables): written by the block that ends the hypothesis
  const int* hyp_out;              // [n_hyp] output id of the hypothesis in each slot
  int* res_tok; int* res_len; float* res_cum;   // [n_out][n_ctx] generated tokens (no prompt), [n_out], [n_out]
  float* res_lp;                   // [n_out][n_ctx] per-step records (with tok_lp; nullptr: none)
  float* res_lp_other;
  // rules over the hypothesis' generated tokens (search.hip header): penalty 1 and n-gram size 0 are off, and
  // launch_logits_select then runs the instantiations without them
  float rep_penalty;               // > 0
  int no_repeat_ngram;             // >= 0
  // ragged prompts (both or neither; nullptr: sample_begin / max_length hold for every hypothesis): the prompt
  // length and the total length limit of the window in each hypothesis slot, [n_hyp], device memory
  const int* hyp_begin;
  const int* hyp_maxlen;
  // sequence bias (search.hip header; n_bias 0: off, and launch_logits_select then runs the instantiations without
  // it): entry j is tokens bias_tok[bias_off[j] .. bias_off[j + 1]) (1 .. SEARCH_BIAS_LEN ids inside the vocabulary)
  // with bias bias_val[j]; the entries are sorted by their LAST token, entries with the same last token in the
  // caller's order.  Device memory.
  const int* bias_off;             // [n_bias + 1]
  const int* bias_tok;
  const float* bias_val;           // [n_bias], finite
  int n_bias;                      // <= SEARCH_BIAS_MAX
  // per-window seeds (sampling only; both or neither; nullptr: `seed` and the call-wide hypothesis index hold):
  // the hypothesis in slot h draws gumbel(hyp_seed[h], hyp_key[h], step, i), hyp_key its index among its own
  // window's hypotheses, so a window's draws do not depend on its place in the call.  [n_hyp], device memory,
  // filled like hyp_begin / hyp_maxlen; launch_logits_select then runs the SEED instantiations of mode 2.
  const unsigned long long* hyp_seed;
  const int* hyp_key;
};

struct BeamParams {
  int beam, max_cand, n_ctx, sample_begin, max_length, eot;
  const int* cand_tok; const float* cand_lp;
  int* tokens; int* lin; int* seq_len; float* cum; int* done;
  int* row_tok; int* row_pos;
  int* fin_tok;          // [n_win][max_cand][n_ctx]  (generated tokens only)
  int* fin_len; float* fin_cum; int* n_fin;   // [n_win][max_cand], [n_win]
  int* n_active;
  // optional per-step records (nullptr: off): tok_lp [n_hyp][n_ctx] log-prob of the token at each position (copied
  // along the lineage like the tokens), fin_lp [n_win][max_cand][n_ctx] a finished hypothesis' records (generated
  // tokens, then its <|endoftext|>)
  float* tok_lp;
  float* fin_lp;
  // ragged prompts, as SearchParams (a window's values are read at its first hypothesis)
  const int* hyp_begin;
  const int* hyp_maxlen;
};

// Row-set decode bookkeeping (engine.cpp generate_rows).  Start hypotheses: slot hs[i] takes window ws[i] (prompt
// win_prompt[ws[i]][0..P) into tokens, seq_len P, live, cum 0, its cross slot and output id).  Ragged prompts
// (win_len != nullptr): P is the row stride of win_prompt, window w's prompt is its first win_len[w] tokens, and the
// slot's rows of the selection tables become hyp_begin[h] = win_len[w], hyp_maxlen[h] = win_maxlen[w].  Per-window
// seeds (win_seed != nullptr): hyp_seed[h] = win_seed[w], hyp_key[h] = 0 (one hypothesis per window).
void launch_hyp_start(int n, const int* hs, const int* ws, const int* win_prompt, int P, const int* win_slot, int n_ctx,
                      int* tokens, int* seq_len, int* done, float* cum, int* hyp_slot, int* hyp_out, hipStream_t st,
                      const int* win_len = nullptr, const int* win_maxlen = nullptr, int* hyp_begin = nullptr,
                      int* hyp_maxlen = nullptr, const unsigned long long* win_seed = nullptr,
                      unsigned long long* hyp_seed = nullptr, int* hyp_key = nullptr);
// Pass rows whose token / position live on the device: row i with src[i] >= 0 takes (row_tok, row_pos)[src[i]].
void launch_rows_fill(int n, const int* src, int* tok, int* pos, const int* row_tok, const int* row_pos, hipStream_t st);
void launch_beam_start(int n, const int* gs, const int* ws, int K, const int* win_prompt, int P, const int* win_slot,
                       int n_ctx, int* tokens, int* lin, int* seq_len, int* done, float* cum, int* hyp_slot, int* n_fin,
                       hipStream_t st, const int* win_len = nullptr, const int* win_maxlen = nullptr,
                       int* hyp_begin = nullptr, int* hyp_maxlen = nullptr);

// dst[dst_row[i]][0..V) = src[i][0..V) for i < n (f32 rows; the ragged prefill's per-class logit rows -> selection order)
void launch_rows_scatter(const float* src, float* dst, const int* dst_row, int n, int V, hipStream_t st);

// one block per row (n_rows = hypotheses, or the compacted row set's rows with p.row_hyp)
void launch_logits_select(const SearchParams& p, int n_rows, hipStream_t st);
// host: the suppress_bits words for a vocabulary of V ids (sup[i] != 0: suppressed)
void search_suppress_bits(const unsigned char* sup, int V, unsigned long long* bits /* [SEARCH_SB] */);
void launch_beam_select(const BeamParams& p, int n_win, hipStream_t st);
// out[r][j] = softmax(logits row r restricted to [lang_begin, lang_begin + n_langs))[j]
void launch_lang_probs(const float* logits, long long ldl, int rows, int lang_begin, int n_langs, float* out, hipStream_t st);
// Language head: row r of x ([rows][ldx] f32, the decoder's last hidden state before dec.ln) -> LayerNorm(g, b) rounded
// to bf16 -> dot products with rows lang_begin .. lang_begin + n_langs - 1 of E ([V][d] bf16) -> optional mask
// (allowed[j] == 0: probability exactly 0; nullptr: all) -> f32 softmax probs[r][n_langs], top_id[r] (lowest index on
// ties), top_prob[r].  A row without a finite allowed logit reports (WM_ERR_NONFINITE, row0 + r) through err.
// d: 384, 512, 768, 1024 or 1280; n_langs <= SEARCH_LANG_MAX.
void launch_lang_head(const float* x, long long ldx, int rows, int d, const float* g, const float* b, const bf16* E,
                      int lang_begin, int n_langs, const unsigned char* allowed, float* probs, int* top_id,
                      float* top_prob, int row0, int* err, hipStream_t st);
// Language assignment (wm_generate_multilingual): table[ent[2i]] = lang_begin + top[ent[2i + 1]] for i < n, where top is
// launch_lang_head's top_id table on the device (an entry whose top is outside [0, n_langs) is skipped).  The caller has
// checked every offset against its table.
void launch_lang_assign(int n, const int* ent, const int* top, int lang_begin, int n_langs, int* table, hipStream_t st);
// out[out_idx ? out_idx[r] : r] = softmax(logits row r)[no_speech]
void launch_no_speech(const float* logits, long long ldl, int V, int rows, int no_speech, float* out, hipStream_t st,
                      const int* out_idx = nullptr);
