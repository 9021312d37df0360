/* whisper_mi355.h — C-ABI of the MI355X (gfx950) Whisper engine, libwhisper_mi355.so.
 *
 * The drop-in boundary is faster-whisper's `WhisperModel(...).transcribe(...)` as the vlog transcription
 * worker calls it (reference `worker/transcription.py:78-111`).  Below that call, faster-whisper drives
 * CTranslate2's C++ `models.Whisper` (encode / generate / detect_language / align) [FW↑]; this library
 * replaces that C++ seam, plus faster-whisper's numpy log-mel.  The Python host (vlog_amd/) mirrors the
 * faster-whisper surface on top of these entry points and owns all input/output device buffers
 * (PyTorch-ROCm tensors); the engine owns the weights, the KV caches and its scratch.
 *
 * Conventions: every function returns 0 on success and -1 on failure (never aborts); the message is
 * available from wm_last_error() (thread-local).  Every call sets the engine's device itself, so calls may
 * come from any thread (the worker runs `transcribe` on a ThreadPoolExecutor thread,
 * worker/transcription.py:361-369); calls on one engine are serialised by an internal lock.  Pointers
 * named d_* are device pointers; h_* are host pointers.  `stream` is a hipStream_t (NULL = null stream).
 */
#ifndef WHISPER_MI355_H
#define WHISPER_MI355_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wm_engine wm_engine;

typedef struct wm_model_dims {
  int32_t n_mels, n_state, n_head, n_enc_layer, n_dec_layer, n_vocab, n_audio_ctx, n_text_ctx;
  int32_t eot, sot, no_speech, no_timestamps, timestamp_begin, blank;
} wm_model_dims;

/* Replaces ctranslate2.models.Whisper(model_path, device, compute_type) as constructed by
 * faster_whisper.WhisperModel.__init__ [FW↑] (called at worker/transcription.py:81-85). */
int wm_create(const wm_model_dims* dims, int32_t device, wm_engine** out);
void wm_destroy(wm_engine* e);
const char* wm_last_error(void);
int32_t wm_abi_version(void);

/* Weight upload into the engine's packed layout (names and layouts: see INTEGRATION.md §Weights).
 * d_src must hold exactly nbytes (bf16 matrices, f32 vectors). */
int wm_set_weight(wm_engine* e, const char* name, const void* d_src, int64_t nbytes, void* stream);
/* 1 when every weight has been set. */
int32_t wm_weights_complete(wm_engine* e);
/* The weights wm_set_weight expects, in layout order (for bindings that do not carry this table, e.g. a C or
 * Go host): name (owned by the engine), size in bytes, element bytes (2 = bf16 matrix, 4 = f32). */
int32_t wm_weight_count(wm_engine* e);
int wm_weight_info(wm_engine* e, int32_t i, const char** name, int64_t* nbytes, int32_t* elem_bytes);

/* Log-mel, replacing faster-whisper FeatureExtractor.__call__ [FW↑] (reached from
 * worker/transcription.py:105).  Computes frames [frame0, frame0+n_frames) of the WHOLE-FILE spectrogram
 * (file of n_samples samples; d_pcm[i] is file sample pcm_offset+i) as log10(max(mel, 1e-10)) into
 * d_mel[m*ld + f], and folds their maximum into *d_gmax (order-preserving uint32, zero-initialised by the
 * caller).  frame0 must be even: frames are transformed in (even, odd) pairs, so any split of a file into
 * even-aligned frame ranges gives bit-identical frames.  wm_logmel_finalize applies max(x, gmax-8), (x+4)/4
 * in place; gmax is taken from h_gmax when non-NULL (cross-shard max), else from d_gmax. */
int wm_logmel(wm_engine* e, const float* d_pcm, int64_t pcm_offset, int64_t n_samples, int64_t frame0,
              int32_t n_frames, float* d_mel, int64_t ld, uint32_t* d_gmax, void* stream);
int wm_logmel_finalize(wm_engine* e, float* d_mel, int64_t n_frames, int64_t ld, const uint32_t* d_gmax,
                       const float* h_gmax, float* h_gmax_out, void* stream);

/* Streaming ingest: n s16le samples (the worker's ffmpeg output, received through a pipe into a pinned
 * buffer and copied to the device) -> f32 x / 32768, faster-whisper decode_audio's conversion.  The caller
 * then runs wm_logmel on the frames whose window lies inside the samples received so far (vlog_amd/ingest.py). */
int wm_pcm_from_s16(wm_engine* e, const int16_t* d_src, int64_t n, float* d_dst, void* stream);

/* Sample-rate conversion to 16 kHz with downmix: interleaved PCM frames at src_rate -> f32 mono, so a producer
 * (ffmpeg) can hand over native-rate, native-channel PCM.  The filter is scipy.signal.resample_poly's default:
 *   g = gcd(16000, rate), up = 16000/g, down = rate/g, m = max(up, down), half = 10 m, N = 2 half + 1 taps
 *   h[k] = (1/m) sinc((k - half)/m) I0(5 sqrt(1 - ((k - half)/half)^2)) / I0(5),  sinc(x) = sin(pi x)/(pi x)
 *   h /= sum(h);  h *= up                  (= scipy.signal.firwin(N, 1/m, window=("kaiser", 5.0)) * up)
 *   mono[i] = mean of the channels of frame i (s16: the exact integer sum times the f32 constant 1/(32768 ch);
 *             f32: the sum in channel order times 1/ch), or one chosen channel; frames outside the file are zero
 *   y[j] = sum_i mono[i] h[j down - i up + half]   over 0 <= i < n_total, tap index in [0, 2 half]
 *   n_out = ceil(n_total up / down); not clipped.  src_rate 16000: up = down = 1, half = 0, the single tap 1.
 * The taps are evaluated in f64, rounded to f32 and cached on the device per ratio; the sum is f32 in a fixed
 * order, so output j is the same bits whatever the call's output range or source span.  Supported: N <= 16384
 * (max(up, down) <= 819: 8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000 Hz
 * among others), 1 .. 8 channels.
 *
 * wm_resample_plan: pure host, no GPU touched: 0, or -1 for an unsupported rate (the message names the rate).
 * wm_resample_taps: the f32 taps the kernel uses, h_taps[2*half_len+1]; pure host.
 * wm_resample: outputs [out0, out0+n_out) of the whole-file resampling into d_dst[0..n_out).  d_src holds source
 * frames [src_offset, src_offset+n_src) (interleaved, fmt 0 = s16, 1 = f32).  channel -1 = mean of all, else that
 * channel.  n_total = frames in the file, or -1 "end not yet known" (streaming).  Output j reads frames
 * ceil((j down - half)/up) .. floor((j down + half)/up), clipped to the file.  Fails (-1, nothing launched) on an
 * unsupported rate, bad channels / channel, a negative length, src_offset + n_src > n_total, out0 + n_out >
 * ceil(n_total up / down), or a needed frame inside the file that the span does not hold (with n_total = -1: any
 * frame at or past src_offset + n_src).  n_out == 0 succeeds and launches nothing. */
int wm_resample_plan(int32_t src_rate, int32_t* up, int32_t* down, int32_t* half_len);
int wm_resample_taps(int32_t src_rate, float* h_taps);
int wm_resample(wm_engine* e, const void* d_src, int32_t fmt, int32_t channels, int32_t channel, int32_t src_rate,
                int64_t src_offset, int64_t n_src, int64_t n_total, int64_t out0, int64_t n_out, float* d_dst, void* stream);

/* Per-frame log energy (dB) of ceil(n_samples / frame) frames, the speech-probability input of the VAD
 * stand-in (faster-whisper's Silero VAD [FW↑], reached via vad_filter=True at worker/transcription.py:110). */
int wm_frame_energy(wm_engine* e, const float* d_pcm, int64_t n_samples, int32_t frame, float* d_db, void* stream);

/* The fp8 cross memory's quantisation (wm_set_option "cross_fp8"), exposed for tests: rows of n_state bf16
 * values -> OCP e4m3 codes of x * 448 / amax_row (round to nearest even) and scale amax_row / 448 per row
 * (an all-zero row: zeros, scale 0).  wm_cross_kv applies it to the window slots when cross_fp8 is on. */
int wm_cross_fp8_quantize(wm_engine* e, const void* d_enc, int64_t rows, uint8_t* d_codes, float* d_scale, void* stream);

/* The quantisation of the projected form's fp8 K/V panels (wm_set_option "cross_kv_fp8"), exposed for tests.  A row is
 * 64 bf16 values: the head_dim values of one (layer, K or V, slot, head, position) as the bf16 panels store them.
 * Per row: 64 OCP e4m3 codes (d_codes [n_rows][64]) and one exponent byte b = e + 127 (d_exp [n_rows]); the stored
 * value is e4m3(code) * 2^e.
 *   - a row with a non-finite value: every code 0x7F (e4m3 NaN), b = 127;
 *   - amax = max |x| == 0: every code 0x00, b = 127;
 *   - otherwise e is the smallest integer with amax * 2^-e <= 448, from the bits of amax = m * 2^k (1 <= m < 2;
 *     448 = 1.75 * 2^8): e = k - 8 if m <= 1.75, else k - 7, clamped to [-110, 110];
 *   - code = round-to-nearest-even of x * 2^-e onto the e4m3 grid, saturating at +-448 (reachable only behind the
 *     upper clamp of e).
 * A dequantised value has at most 4 significant bits and is a normal number, so it is exactly a bf16 value: the fp8
 * attention kernels compute on exactly the values a bf16 panel of the dequantised rows would hold.
 * (Added without an ABI bump: a new entry point only.) */
int wm_cross_kv_fp8_quantize(wm_engine* e, const void* d_rows_bf16, int64_t n_rows, uint8_t* d_codes, uint8_t* d_exp,
                             void* stream);

/* Silero VAD v5 (16 kHz) network weights, f32 device pointers in PyTorch layouts: STFT basis [258][256],
 * encoder convs conv_w[i] [out][in][3] with (in, out) = (129,128), (128,64), (64,64), (64,128) and biases
 * [out], LSTMCell w_ih/w_hh [512][128] (gate order i, f, g, o) and b_ih/b_hh [512], head conv1x1 [128] + [1]. */
typedef struct wm_vad_weights {
  const float* stft_basis;
  const float* conv_w[4];
  const float* conv_b[4];
  const float* w_ih;
  const float* w_hh;
  const float* b_ih;
  const float* b_hh;
  const float* head_w;
  const float* head_b;
} wm_vad_weights;

/* Speech probability of each 512-sample window of d_pcm (n_samples a multiple of 512; the caller pads as
 * faster-whisper's get_speech_timestamps does), replacing faster-whisper 1.1 SileroVADModel.__call__ [FW↑
 * vad.py] — its batched encoder (each window prefixed with the previous window's last 64 samples, zeros for
 * the first) and its sequential LSTM decoder with h, c starting at zero.  d_work: 512 * n_samples/512 floats
 * of scratch; d_probs: n_samples/512 floats. */
int wm_vad_probs(wm_engine* e, const wm_vad_weights* w, const float* d_pcm, int64_t n_samples, float* d_work,
                 float* d_probs, void* stream);

/* Encoder, replacing ctranslate2 Whisper.encode(features) [FW↑] (faster-whisper generate_segments).
 * Window b reads mel frames [h_seek[b], h_seek[b]+h_nframes[b]) of d_mel (ld = frames per mel row) and
 * zero-pads to 3000 frames (faster-whisper pad_or_trim).  Output bf16 [B][1500][n_state]. */
int wm_encode(wm_engine* e, const float* d_mel, int64_t ld, const int32_t* h_seek, const int32_t* h_nframes,
              int32_t B, void* d_enc_out, void* stream);

/* Capacity of the decoder state: n_slots windows (encoder outputs, or cross-KV panels with cross_mode 0),
 * n_hyp hypotheses of self-KV. */
int wm_reserve(wm_engine* e, int32_t n_slots, int32_t n_hyp, void* stream);

/* Makes B encoder outputs the cross-attention memory of slots [slot0, slot0+B) (CTranslate2 projects them
 * to K/V inside generate [FW↑]).  Default (factored cross-attention): the slot keeps the encoder output
 * itself and the decoder attends over it (q' = Wk_h^T q, u = P E, Wv after the merge).  cross_mode 0: the
 * K/V projection of all decoder layers is computed here (with cross_kv_fp8 on, chunk by chunk through the
 * quantiser: see the option). */
int wm_cross_kv(wm_engine* e, const void* d_enc, int32_t B, int32_t slot0, void* stream);

/* ctranslate2 Whisper.generate(encoder_output, prompts, ...) [FW↑] as faster-whisper
 * generate_with_fallback calls it: greedy (beam_size 1, temperature 0), beam search (beam_size > 1, patience,
 * length_penalty) or sampling (temperature > 0, num_hypotheses = best_of).  Logit rules, log-softmax and selection
 * run on the device.
 * Shared by all windows of one call: the decode form and its parameters (beam_size, patience, length_penalty,
 * temperature, num_hypotheses, seed), the logit rules (suppress list, suppress_blank, max_initial_timestamp_index,
 * with_timestamps, repetition_penalty, no_repeat_ngram_size) and the scheduling fields (check_every, max_rows,
 * compact).  Per window: the cross-KV slot, the prompt and, since ABI 4, its length (h_prompt_lens), the position
 * its no-speech probability is read at (h_sot_indices) and its total length limit (h_max_lengths), so windows
 * whose previous-text prompts differ in length (faster-whisper's condition_on_previous_text, one file per window)
 * decode in the same passes.  Each window's result is what a call with that window alone computes, to the f32
 * rounding of the pass's GEMM / attention routes (which follow the pass's row count).  (Sampling: with the one
 * `seed` of this struct a window's draws follow its place in the call; wm_generate_seeded takes a seed per window.) */
typedef struct wm_generate_args {
  int32_t n_windows;
  const int32_t* h_slots;        /* [n_windows] cross-KV slot of each window */
  int32_t prompt_len;            /* prompt length of every window (ABI 4 h_prompt_lens: the row stride of h_prompts) */
  const int32_t* h_prompts;      /* [n_windows][prompt_len] */
  int32_t sot_index;             /* position of <|startoftranscript|> in the prompt; -1: no no_speech_prob */
  int32_t beam_size;
  float patience;
  float length_penalty;
  int32_t max_length;            /* total decoder length including the prompt (<= n_text_ctx) */
  float temperature;             /* > 0: sampling */
  int32_t num_hypotheses;        /* sampling: best_of */
  uint64_t seed;
  const int32_t* h_suppress;     /* suppressed token ids */
  int32_t n_suppress;
  int32_t suppress_blank;
  int32_t max_initial_timestamp_index;   /* < 0: none */
  int32_t with_timestamps;
  int32_t check_every;           /* steps between host checks for completion (>= 1) */
  /* outputs (host) */
  int32_t* h_tokens;             /* [n_windows][max_length] generated tokens (no prompt, no <|endoftext|>) */
  int32_t* h_lengths;            /* [n_windows] */
  float* h_scores;               /* [n_windows] cum_logprob / len^length_penalty (CTranslate2 score) */
  float* h_cum_logprob;          /* [n_windows] */
  float* h_no_speech;            /* [n_windows] */
  int32_t* h_steps;              /* [1] decoder steps run (incl. prefill) */
  /* ---- ABI 2 (wm_abi_version() >= 2) */
  /* Row-set decode (greedy, or sampling with num_hypotheses 1): at most max_rows windows decode at once (0: all);
   * when one ends, its row takes the next window in h_slots order at the next host check (the new window's prompt
   * is prefilled inside that step's decoder pass), so the step count follows the total work instead of the longest
   * window.  Order the windows longest-expected first (vlog_amd/shard.py expected_tokens).  compact = 1: once no
   * window is waiting, finished rows are dropped from the passes when the live rows fall to 7/8 of the pass (the
   * step graph is re-captured for the new row count).  Each window's result is the same computation either way;
   * the GEMM / attention routes follow the pass's row count, so results agree to f32 rounding, not bit for bit.
   * Beam search: max_rows (a multiple of beam_size is used: max_rows / beam_size windows in flight) refills a
   * finished window's group of beam_size rows with the next window (no per-step records in this form); compact = 1
   * drops the hypotheses of finished windows from the passes once nothing waits (when the live hypotheses fall to
   * 7/8 of the pass). */
  int32_t max_rows;
  int32_t compact;
  /* Optional per-step records, [n_windows][max_length] (NULL: off): the log-prob (after the logit rules) of the
   * token chosen at each generated step, the final <|endoftext|> included (h_lengths[w] + 1 entries when the window
   * ended on it, else h_lengths[w]); and, greedy / sampling, the best log-prob among the other allowed tokens at that
   * step.  Beam search records the chosen hypothesis' path. */
  float* h_token_logprobs;
  float* h_token_logprobs_other;
  /* Optional statistics [4] (NULL: off): decoder passes, sum over decode passes of the rows in the pass, windows
   * started after the first pass (refills), step graphs captured. */
  int64_t* h_stats;
  /* ---- ABI 3 (wm_abi_version() >= 3) */
  /* Two logit rules over each hypothesis' GENERATED tokens (never the prompt, previous text, prefix or hotwords),
   * applied on the device to the raw logits before every other rule, so they also feed the timestamp forcing and the
   * log-prob normaliser.  They restate CTranslate2's repetition_penalty / no_repeat_ngram_size of Whisper.generate
   * [FW↑] from their documented behaviour (parity with CTranslate2 is unpinned: it is not a dependency here).
   * repetition_penalty p > 0: the logit x of every id already generated becomes x < 0 ? x * p : x / p (timestamps
   * included); 0 and 1 are off.  no_repeat_ngram_size n >= 1: an id that would complete an n-gram already among the
   * generated tokens is masked (n = 1: every generated id); 0 is off.  Zero in both fields keeps the ABI 2 behaviour
   * (a zero-filled struct is valid).  A negative or non-finite penalty, n < 0 or n > max_length fails the call; a
   * row the rules leave without a legal token fails it as in the failure contract below.  Every decode form applies
   * them (greedy, sampling, beam, the row-set decodes: a refilled row's history restarts with its new window). */
  float repetition_penalty;
  int32_t no_repeat_ngram_size;
  /* ---- ABI 4 (wm_abi_version() >= 4) */
  /* Ragged prompts: per-window prompt length, sot position and length limit, each [n_windows] or NULL.  A zero-filled
   * tail (three NULLs) keeps the ABI 3 behaviour exactly, and launches the same kernels.
   * h_prompt_lens: NULL: every window's prompt is prompt_len tokens.  Otherwise prompt_len is the row stride of
   * h_prompts and window w's prompt is the first h_prompt_lens[w] tokens of its row; the padding behind it is neither
   * validated nor read.
   * h_sot_indices: NULL: sot_index holds for every window.  Otherwise window w's no-speech probability is read at its
   * own position h_sot_indices[w] (< 0: none for that window, h_no_speech[w] = 0).
   * h_max_lengths: NULL: max_length holds for every window.  Otherwise h_max_lengths[w] is the total decoder length
   * of window w including its prompt (faster-whisper's max_new_tokens is len(prompt) + max_new_tokens per window).
   * max_length stays the row stride of h_tokens and of the record arrays and must be >= every entry.
   * The call fails (-1, before anything is launched, the message names the window) on a prompt length <= 0 or
   * > prompt_len, a prompt length >= that window's max length, a max length > n_text_ctx or > max_length, a sot index
   * >= that window's prompt length, or a token outside the vocabulary inside a prompt.  Every decode form takes
   * ragged prompts (greedy, sampling with any num_hypotheses, beam search; max_rows 0, max_rows below the windows,
   * compact); the rules of ABI 3 start at each window's own prompt length, and the sampling step index counts the
   * window's own generated tokens.  The logit rules, the seed and the decode form stay shared.  h_steps / h_stats keep
   * their meaning. */
  const int32_t* h_prompt_lens;
  const int32_t* h_sot_indices;
  const int32_t* h_max_lengths;
} wm_generate_args;
/* Failure contract: a NaN / inf logits row or a row whose rules allow no token, detected on the device, fails the
 * call (-1, wm_last_error names the window and step) instead of emitting a token. */
int wm_generate(wm_engine* e, const wm_generate_args* a, void* stream);

/* wm_generate with one sampling seed per window (the sequential mode's fallback ladder decoded by levels: the windows
 * of several files or sections that failed temperature i re-decode together, each with its own file's seed
 * window + i).  h_seeds == NULL, or a->temperature <= 0: exactly wm_generate(e, a, stream), the same kernels and
 * the same bits.  Otherwise hypothesis j (0 <= j < num_hypotheses) of window w draws its Gumbel noise at its own
 * decode step s and token i from (h_seeds[w], j, s, i) and a->seed is not read: the noise depends on the window's
 * seed and the hypothesis' index inside its window, never on the window's place in the call.  The result of window w
 * is therefore what a call with that window alone and seed = h_seeds[w] computes, to the f32 rounding of the pass's
 * GEMM / attention routes (the guarantee ragged prompts give).  Every form that samples takes the seeds: the lockstep
 * decode with any num_hypotheses, and the row-set forms (num_hypotheses 1 with max_rows below the windows, or
 * compact), whose key (seed, w) becomes (h_seeds[w], 0).  The seeds live in per-hypothesis device tables filled once
 * per call (row-set: when a slot takes a window), so no launch is added per step and captured step graphs stay valid;
 * only the sampling selection has instantiations that read them.  Any u64 is a valid seed; validation, the failure
 * contract, h_steps and h_stats are wm_generate's.  (Added without an ABI bump: a new entry point, wm_generate_args
 * unchanged.) */
int wm_generate_seeded(wm_engine* e, const wm_generate_args* a, const uint64_t* h_seeds /* [n_windows] or NULL */,
                       void* stream);

/* Sequence bias: the third rule over each hypothesis' GENERATED tokens (transformers' SequenceBiasLogitsProcessor):
 * custom-vocabulary boosts and soft or hard bans.  The table has n entries; entry j is the token sequence
 * h_tokens[h_off[j] .. h_off[j+1]) of 1 .. 16 ids inside the vocabulary, with the finite bias h_bias[j].  At a
 * decode step of a hypothesis with G generated tokens (the tokens after that window's own prompt: never the prompt,
 * previous text, prefix or hotwords), entry j of length n_j is active iff n_j - 1 <= G and the last n_j - 1
 * generated tokens equal the entry's first n_j - 1 ids (entries of length 1 are always active); every active entry
 * adds its bias to the logit of its LAST id.  Active entries that end in one id add up in entry order (f32, the sum
 * first, then the logit), so a run is reproducible bit for bit; duplicates are allowed.  Only the completing token is
 * biased: to favour a multi-token name from its first token, list its prefixes as entries of their own.
 * Order: repetition penalty, sequence bias, no-repeat n-gram mask, then suppression, blank and timestamp rules.  So
 * the bias feeds the timestamp forcing and the log-prob normaliser: h_scores, h_cum_logprob, the per-step records
 * and the beam ranking are those of the BIASED distribution.  A mask wins over a bias (a masked id stays masked).
 * The table belongs to the engine: it holds for every later wm_generate, in all decode forms (greedy, sampling,
 * beam, the row-set decodes, ragged prompts), until it is replaced; n = 0 clears it (the pointers may be NULL), and
 * an engine without a table launches exactly the kernels it launched before this entry point existed.
 * The call fails (-1, nothing launched, wm_last_error names the entry) on n > 1024, offsets that do not start at 0
 * or do not ascend, an empty entry or one of more than 16 tokens, an id outside the vocabulary or a non-finite
 * bias; the previous table then stays in place and the engine usable.  The upload is ordered on `stream` and
 * complete when the call returns.  No per-step launch is added.  (Added without an ABI bump: a new entry point,
 * wm_generate_args unchanged.) */
int wm_set_sequence_bias(wm_engine* e, int32_t n, const int32_t* h_off /* [n + 1] */, const int32_t* h_tokens,
                         const float* h_bias /* [n] */, void* stream);

/* Teacher-forced decoder forward over n_seq sequences of seq_len tokens (one window slot each): logits for
 * every position (d_logits f32 [n_seq*seq_len][n_vocab]) or only the last (last_only: [n_seq][n_vocab]).
 * Optional cross-attention capture for word alignment (ctranslate2 Whisper.align [FW↑]): for each of
 * n_align (layer, head) pairs in h_align_heads, softmax weights are written to
 * d_attn[((s*seq_len + p)*n_align + a)*1500 + t].  Also serves detect_language ([sot], last_only). */
int wm_forward(wm_engine* e, int32_t n_seq, const int32_t* h_slots, int32_t seq_len, const int32_t* h_tokens,
               float* d_logits, int32_t last_only, const int32_t* h_align_heads, int32_t n_align, float* d_attn,
               void* stream);

/* ctranslate2 Whisper.detect_language(encoder_output) [FW↑] (faster-whisper detect_language, reached from
 * worker/transcription.py:105-111 with language=None): one decoder step from <|startoftranscript|> for each of n
 * windows (slots h_slots), softmax over the n_langs language tokens starting at lang_begin, on the device.
 * h_probs [n][n_langs], in language-token order. */
int wm_detect_language(wm_engine* e, int32_t n, const int32_t* h_slots, int32_t lang_begin, int32_t n_langs,
                       float* h_probs, void* stream);

/* Language identification of n windows (slots h_slots, any order, repeats allowed) in one call, optionally restricted
 * to a set of candidate languages: one decoder step from <|startoftranscript|> per row, then a language head on the
 * device that reads only rows lang_begin .. lang_begin + n_langs - 1 of the tied embedding (no [n][n_vocab] logits
 * buffer is allocated or written).  Per row: the final LayerNorm in f32 rounded to bf16 as the logits GEMM's operand
 * is, the n_langs dot products (f32 sums of the same bf16 x bf16 products wm_detect_language sums, in another order),
 * the mask, an f32 softmax over the languages left, and the argmax (the lowest index wins ties).
 *   h_allowed   [n_langs] bytes or NULL (= all): language j takes part iff h_allowed[j] != 0; the probabilities are
 *               renormalised over the allowed languages and a masked language's probability is exactly 0.0f.
 *   h_probs     [n][n_langs] in language-token order; h_top [n] the best language's index (0-based from
 *               lang_begin); h_top_prob [n] its probability.
 * Rows are decoded 160 per pass in call order.  The call fails before any launch, naming the argument, when
 * lang_begin .. lang_begin + n_langs leaves the vocabulary, n_langs is outside 1..128, h_allowed sets no language or
 * a slot is outside the reserved ones; it fails with "wm_language_id: non-finite logits, row r" when row r has no
 * finite logit among its allowed languages.  wm_detect_language is unchanged and stays the full-vocabulary form. */
int wm_language_id(wm_engine* e, int32_t n, const int32_t* h_slots, int32_t lang_begin, int32_t n_langs,
                   const uint8_t* h_allowed /* [n_langs] or NULL = all */, float* h_probs /* [n][n_langs] */,
                   int32_t* h_top /* [n] */, float* h_top_prob /* [n] */, void* stream);

/* wm_generate_seeded whose windows choose their own language on the device (faster-whisper's multilingual=True: every
 * 30 s window is decoded under the language detected for it).  The "auto" windows are those with h_lang_pos[w] >= 0,
 * in call order.  Before the first prefill they are identified exactly as wm_language_id identifies that sub-list of
 * slots (160 rows per pass in call order, the same decoder step and language head, the one mask h_allowed for the
 * whole call), so h_lang, h_lang_prob and h_probs carry the bits of that call.  The best indices stay on the device,
 * and a kernel (lang_assign_kernel) writes the token lang_begin + h_lang[w] at position h_lang_pos[w] of window w's
 * prompt in every device table that holds it (each hypothesis' token row and the prefill rows; the row-set forms'
 * per-window prompt table and, at a refill, the starting windows' pass rows), ordered on the stream after those
 * tables' uploads and before the pass that prefills them.  Every window is identified at the start of the call, the
 * row-set forms' later windows too (their cross K/V is in its slot already).  No host wait is added between the
 * detection and the prefill: the results' copy back is queued behind the language head and is delivered when the call
 * returns.  From the assignment on the call is wm_generate_seeded with host prompts that hold those tokens: tokens,
 * scores, cum_logprob, no-speech, the per-step records, h_steps and h_stats are bit-identical to it for the same
 * windows, order and options, in every decode form (greedy, sampling with any num_hypotheses, with or without seeds,
 * beam search, ragged prompts, the row-set forms with max_rows below the windows and with compact).
 *   h_lang_pos   [n_windows]: the prompt position whose token the engine replaces; -1: the window keeps its prompt.
 *                The host puts a placeholder language token there, right behind <|startoftranscript|>.
 *   h_lang       out [n_windows]: the chosen index from lang_begin; -1 where h_lang_pos is -1
 *   h_lang_prob  out [n_windows]: its probability; 0 where h_lang_pos is -1
 *   h_probs      out [n_windows][n_langs] or NULL; zeros where h_lang_pos is -1
 * la == NULL is exactly wm_generate_seeded(e, a, h_seeds, stream).  The call fails before any launch, naming the
 * window, when h_lang_pos[w] is at or beyond that window's prompt length, the token there is not a language token in
 * [lang_begin, lang_begin + n_langs), or the token before it is not <|startoftranscript|>; and, as wm_language_id,
 * when n_langs is outside 1..128, the language tokens leave the vocabulary or h_allowed sets no language.  A window
 * without a finite allowed language logit fails the call ("non-finite language logits, window w") after the decode;
 * its prompt kept the placeholder.  The engine stays usable after a refusal, and an engine that never makes this call
 * launches exactly what it launched before.  (Added without an ABI bump: a new entry point, wm_generate_args
 * unchanged.) */
typedef struct wm_language_auto {
  int32_t lang_begin, n_langs;      /* as wm_language_id */
  const uint8_t* h_allowed;         /* [n_langs] or NULL = all (one mask per call) */
  const int32_t* h_lang_pos;        /* [n_windows] */
  int32_t* h_lang;                  /* out [n_windows] */
  float* h_lang_prob;               /* out [n_windows] */
  float* h_probs;                   /* out [n_windows][n_langs] or NULL */
} wm_language_auto;
int wm_generate_multilingual(wm_engine* e, const wm_generate_args* a, const wm_language_auto* la /* or NULL */,
                             const uint64_t* h_seeds /* [n_windows] or NULL */, void* stream);

/* ctranslate2 Whisper.align(encoder_output, start_sequence, text_tokens, num_frames, median_filter_width)
 * [FW↑] for ONE window (faster-whisper find_alignment, word_timestamps=True): teacher-forced decoder pass over
 * h_sot + <|notimestamps|> + h_text + <|endoftext|> with the n_heads (layer, head) alignment heads'
 * cross-attention captured, text-token probabilities, z-score + median filter + head mean, DTW on the
 * device.  Outputs: h_probs[n_text], the DTW path (h_text_idx, h_time_idx) of *h_path_len entries
 * (capacity n_text + 1 + num_frames/2). */
int wm_align(wm_engine* e, int32_t slot, int32_t sot_len, const int32_t* h_sot, int32_t n_text, const int32_t* h_text,
             int32_t num_frames, const int32_t* h_heads, int32_t n_heads, int32_t median_filter_width, float* h_probs,
             int32_t* h_text_idx, int32_t* h_time_idx, int32_t* h_path_len, void* stream);
/* wm_align over a batch of windows (faster-whisper add_word_timestamps over a batch of segments, as the
 * batched pipeline runs it; one teacher-forced decoder pass per chunk of windows and one batched DTW launch
 * instead of one wm_align per window).  Item i: window slot h_slots[i], text tokens
 * h_text[h_text_off[i] .. h_text_off[i+1]), h_num_frames[i] mel frames.  Outputs: probabilities at
 * h_probs[h_text_off[i] + k]; DTW path of item i at h_text_idx / h_time_idx + h_path_off[i] (capacity
 * n_text_i + 1 + num_frames_i / 2), length h_path_len[i]. */
int wm_align_batch(wm_engine* e, int32_t n, const int32_t* h_slots, int32_t sot_len, const int32_t* h_sot,
                   const int32_t* h_text_off, const int32_t* h_text, const int32_t* h_num_frames, const int32_t* h_heads,
                   int32_t n_heads, int32_t median_filter_width, float* h_probs, const int64_t* h_path_off,
                   int32_t* h_text_idx, int32_t* h_time_idx, int32_t* h_path_len, void* stream);
/* DTW alone on a device cost matrix d_cost[n][m] (openai dtw semantics); path as for wm_align. */
int wm_dtw(wm_engine* e, const float* d_cost, int32_t n, int32_t m, int32_t* h_text_idx, int32_t* h_time_idx,
           int32_t* h_path_len, void* stream);
/* The open-end form of wm_dtw (forced alignment: a window may be handed more text rows than its audio holds, so
 * the path may stop at any row).  The same recurrence, f32 arithmetic, tie rules and trace as wm_dtw; then
 * R = the smallest i in [1, n] that minimises cost[i][m], the backtrace starts at (R, m) instead of (n, m), and
 * *h_rows = R ("rows reached": the path visits rows 0 .. R-1 and every column).  No length normalisation: the
 * alignment matrix is the negated per-frame z-score, every column has mean 0 over the rows, so rows whose audio
 * lies beyond the window add positive cost and stopping early leaves negative cost unused.  Path capacity n + m.
 * A minimum that is not finite (NaN or infinity in d_cost) fails the call with "non-finite alignment cost"
 * and writes nothing.  (Added without an ABI bump: new entry points only.) */
int wm_dtw_open(wm_engine* e, const float* d_cost, int32_t n, int32_t m, int32_t* h_text_idx, int32_t* h_time_idx,
                int32_t* h_path_len, int32_t* h_rows, void* stream);
/* wm_align_batch with the open-end DTW (wm_dtw_open) in place of the closed one: the same teacher-forced pass,
 * capture, text-token probabilities and matrix kernels; item i's path ends at row h_rows[i] - 1 of its
 * n_text_i + 1 rows (h_rows [n]; h_rows[i] == n_text_i + 1 gives wm_align_batch's path).  Path capacity per item
 * stays n_text_i + 1 + num_frames_i / 2.  An item whose minimum end cost is not finite fails the call, naming it. */
int wm_align_open_batch(wm_engine* e, int32_t n, const int32_t* h_slots, int32_t sot_len, const int32_t* h_sot,
                        const int32_t* h_text_off, const int32_t* h_text, const int32_t* h_num_frames,
                        const int32_t* h_heads, int32_t n_heads, int32_t median_filter_width, float* h_probs,
                        const int64_t* h_path_off, int32_t* h_text_idx, int32_t* h_time_idx, int32_t* h_path_len,
                        int32_t* h_rows, void* stream);

/* Encoder self-attention kernel alone (diagnostics / parity tests; wm_encode runs it per layer):
 * d_qkv bf16 [B][T][3 n_state] (q | k | v, head h at columns h*64), d_out bf16 [B][T][n_state]. */
int wm_encoder_attention(wm_engine* e, const void* d_qkv, void* d_out, int32_t B, int32_t T, void* stream);

/* Bytes of device memory held by the engine (weights + caches + scratch). */
int64_t wm_device_bytes(wm_engine* e);

/* Built-in kernel profiler (used by bench.py for the live roofline numbers): when enabled, every launch
 * of a kernel class is bracketed by HIP events on its own stream, and the class accumulates its
 * algorithmic FLOPs and bytes (the decoder attention kernels count the K/V bytes they actually read).
 * wm_profile(e, 1) resets and enables, wm_profile(e, 0) disables; wm_profile_read returns launches,
 * summed event time, FLOPs and bytes of one class. */
int32_t wm_profile_classes(void);
const char* wm_profile_name(int32_t cls);
int wm_profile(wm_engine* e, int32_t enable);
/* Engine options (no reference counterpart: scheduling knobs of this build only).  The keys below are the rows of
 * one table in engine.cpp (kOptions) plus the two per-projection forms; any other key fails with "unknown option".
 * Some have an environment variable (named in that table) that overrides the default at wm_create; its integer
 * value goes through the same setter as wm_set_option, so a value the setter rejects (VLOG_AMD_DEC_BIG_LDS=100)
 * makes wm_create fail with the setter's message instead of being clamped.
 *   "cross_mode" (default 1): 1 = factored cross-attention over the encoder output (attn_xenc.hip),
 *   0 = projected cross-KV panels (attn_dec.hip).  Switching re-allocates the window slots (their content is
 *   dropped: call wm_cross_kv again).  The two forms agree to bf16 rounding (not bit-identical).
 *   "decode_split" (default 0): decode steps with >= 32 rows run as two row slices on two streams, one
 *   slice's weight GEMMs overlapping the other's cross-attention.  Results are bit-identical
 *   either way; off by default because the overlap measured slower on MI355X (the GEMM blocks queue behind
 *   the cross-attention blocks).
 *   "decode_graph" (default 1): after one eager decode step, wm_generate captures a step (decoder pass +
 *   token selection) as a HIP graph and replays it for the remaining steps (every per-step quantity lives in
 *   device memory).  Bit-identical either way; off while the event profiler is on or with "decode_split".
 *   "decode_gemv" (default 1): passes of <= 32 decoder rows (one window's beam, a few windows) run every
 *   projection on the small-M weight-streaming GEMM (gemm_dec.hip gemv_dec_kernel); it agrees with the other
 *   routes to f32 rounding.  "decode_gemv_ln" (default 1): passes of <= 16 rows compute the LayerNorms after the
 *   out and cout projections inside the cq / fc1 GEMMs (from the residual and the per-tile row sums and sums of
 *   squares about the tile means that the producers write: a two-pass-equivalent variance) instead of two combine
 *   launches per layer; agrees with the unfused form to f32 rounding.  "decode_gemv_ln_fc2" (default 0): 1 = also
 *   fc2 writes the residual and its row statistics without split-K (16-wave blocks over K = 4 d) and the next layer's
 *   qkv GEMM applies ln1 to its operand (one combine launch fewer per layer; measured ~5 % slower per decoder pass).
 *   "decode_ring_gemm" (default 1): 0 disables the all-rows ring GEMM (plan value 0 below falls back to the
 *   split-K skinny GEMM).
 *   "decode_gemm_plan" (default 1): preset routing of the six decoder projections (qkv, out, cq, cout, fc1, fc2)
 *   for passes of <= 1024 rows; 0 = round-1 routing (ring for qkv/fc1, skinny split-K for the rest), 1 = the
 *   per-projection fastest at 150 rows (tools/dec_gemm_bench; fc1 and fc2 as 64 x 64 ring tiles).  "decode_gemm.<proj>" sets one projection:
 *   > 0 ring GEMM with the rows in groups of that many, 0 all-rows ring, -1 skinny split-K, -2 one-shot GEMM.
 *   Routes differ in K summation order (results agree to f32 rounding, not bit for bit).
 *   "decode_gemm_cols.<proj>" (preset 1: 64 for fc1 and fc2, else 32): output columns per ring-GEMM block, 32 or 64 (64
 *   takes row groups of at most 64; other routes ignore it).  Bit-identical either way.  decode_gemm_plan also
 *   resets these to its preset.
 *   "decode_gemm_big_rows" (default 161): passes of at least this many rows (<= 1024; beam groups of many windows)
 *   route every projection to 64-row ring groups over its whole K (64 columns for qkv / fc1 / fc2, and for all from
 *   512 rows; 0 disables).  Results agree to f32 rounding.
 *   "decode_gemm_big128" (default 512; 0 = never): passes of at least this many rows on that route take the 8-wave
 *   plan: qkv, fc1 and fc2 as 128-row x 128-column blocks, the d x d projections as 64 x 64 (one block of 8 waves per
 *   CU).  Bit-identical to the 4-wave route (same K order per row) except fc2's K ranges below.
 *   "decode_gemm_big_fc2_kr" (default 1280): fc2's K range per block on the 8-wave plan (0 = the whole K, bit-identical
 *   to the 4-wave route; a split sums its slabs in the residual + LayerNorm combine: f32 rounding).
 *   "decode_gemm_big_lds" (default 72): LDS budget in KiB of the qkv / fc1 / fc2 ring blocks on that route, 72 (two
 *   resident blocks per CU) or 144 (one; the d x d projections always take 144).  Bit-identical either way.
 *   "align_fused" (default 1, process-wide): word alignment's z-score + median filter as one statistics kernel and
 *   one wave-per-row-segment median kernel that recomputes z from the attention (never stored); 0 runs the two-kernel
 *   form that writes z.  Bit-identical.
 *   "gemm_persistent" (default 0, process-wide): 1 runs large encoder GEMMs as one persistent block per CU
 *   walking its tiles, the next tile's first K-tiles loaded during the current tile's last K-steps and epilogue
 *   (measured no faster than one block per tile).  Bit-identical.
 *   "cross_attn_keep" (default 0): the factored cross-attention loads the encoder output of the first that many
 *   windows with the default cache policy and the rest non-temporally (an Infinity Cache residency experiment;
 *   measured no gain).  Bit-identical.
 *   "cross_attn_snake" (default 0): odd decoder layers walk the factored cross-attention's items in reverse, so
 *   the encoder output read last by one layer is read first by the next (Infinity Cache reuse).  Bit-identical.
 *   "cross_attn_blocks" (default 0): grid cap of the cross-attention kernel, which walks its
 *   (window, head, key split) items with a grid stride; 0 launches one block per item.
 *   "cross_attn_fuse" (default 1): bit 0 folds the cq projection's split-K combine into the cross-attention
 *   kernel's q load (the q' kernel's, in the factored form); bit 1 combines the key splits in-kernel (last-arriving split) instead of a combine
 *   launch.  Every setting of these three knobs gives bit-identical results.
 *   "encode_chunk" (default 160): windows per encoder pass inside wm_encode (~52 MB of activation scratch
 *   per large-v3 window).
 *   "cross_fp8" (default 0): opt-in fp8 (OCP e4m3) cross memory in the factored form (changes numerics).
 *   "cross_kv_fp8" (default 0; VLOG_AMD_CROSS_KV_FP8): opt-in fp8 K/V panels of the PROJECTED form (cross_mode 0),
 *   independent of cross_fp8: each knob governs its own form.  0 = bf16 panels (the same allocations and kernels as
 *   without the option).  1 = e4m3 codes plus one exponent byte per 64-value row (the format of
 *   wm_cross_kv_fp8_quantize): the slots take (64 + 1) / 128 of the bf16 bytes and every kernel that reads projected
 *   panels converts a code to its exact bf16 value on load (changes numerics against 0).  2 = reference form for
 *   tests and A/B: the same quantiser, the panels stored dequantised as bf16 and read by the bf16 kernels; 1 and 2
 *   hold the same values.  In 1 and 2 wm_cross_kv projects 2 windows at a time into a bf16 staging buffer (2 x
 *   245.8 MB = 491.5 MB at large-v3; a call with one window stages one, 245.8 MB) and quantises them into their
 *   slots.  wm_destroy frees the staging and the exponent bytes with the slots.  Any other value is rejected.  Switching
 *   re-allocates the window slots like cross_mode (their content is dropped: call wm_cross_kv again).
 *   "cross_tf" (default 1): the teacher-forced passes of wm_align / wm_align_batch (projected form) run the
 *   cross-attention on the matrix cores (bf16 MFMA, f32 scores and captured probabilities; the attention weights
 *   enter the V product as bf16); 0 = the f32 VALU kernels of the decode path.
 *   "cross_mfma" (default 1): projected form, decode passes whose windows have 2..32 rows (beam hypotheses, prompt
 *   prefill) run the cross-attention on the same matrix-core kernel, the keys split over blocks to fill the chip and
 *   merged by the split-combine kernel; 0 = the f32 VALU group kernel.  Changes numerics at bf16-rounding level.
 *   "cross_mfma_fuse" (default 0): 1 = that merge done inside the kernel by the last-arriving key split (same
 *   arithmetic and order, bit-identical output; measured ~6 % slower per cross-attention than the separate kernel).
 *   "debug_nan_row" (default -1, TEST ONLY): >= 0 overwrites logits row r of every decode pass of wm_generate with
 *   NaN before token selection (exercises the failure contract of wm_generate).
 *   "debug_nan_count" (default 1, TEST ONLY): the number of consecutive rows from "debug_nan_row" (a whole beam group
 *   gives that window no live candidate). */
int wm_set_option(wm_engine* e, const char* key, int64_t value);
/* The engine's current value of an option (every key wm_set_option accepts, incl. environment overrides). */
int wm_get_option(wm_engine* e, const char* key, int64_t* value);
/* As wm_profile(e, 1) but only the classes whose bit is set in class_mask are timed (0 disables), so a
 * timed run can keep events on the dominant kernel alone. */
int wm_profile_select(wm_engine* e, uint32_t class_mask);
int wm_profile_read(wm_engine* e, int32_t cls, int64_t* launches, double* ms, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif
