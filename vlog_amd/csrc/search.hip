// On-device decoding search for gfx950: Whisper logit rules + log-softmax + greedy / sampling / beam
// candidate selection, and per-window beam bookkeeping.  Restates what CTranslate2's Whisper generate does
// on the host side of each step [FW↑] (oracle: oracle/decode.py; timestamp rules pinned against
// transformers WhisperTimeStampLogitsProcessor):
//   1. SuppressBlank (first sampled step: " " and <|endoftext|>), 2. SuppressTokens (mask), 3. timestamp
//   rules (no <|notimestamps|>; pairs; monotonic; first token a timestamp <= max_initial; if the timestamp
//   log-mass beats the best text token, only timestamps remain).
// One 1024-thread workgroup per hypothesis row streams the 51,866-wide logits row twice (max, then
// sum-exp) per segment (text / timestamps), so the forcing rule and the final normaliser come out of two
// segment log-sum-exps without a third pass.  Greedy and sampling (Gumbel-max over logits / T) update the
// sequence state in the same kernel; beam search emits each hypothesis's top beam+1 candidates and a
// per-window kernel ranks them (openai BeamSearchDecoder semantics, patience, finished list).
//
// Two optional rules act on the raw logits BEFORE all of the above (so they also feed the timestamp forcing and the
// normaliser), restating CTranslate2's RepetitionPenalty and NoRepeatNgram logit processors from their documented
// behaviour; CTranslate2 is not a dependency of this project, so parity with it is unpinned like the rest of
// DESIGN.md §4 (the pinned reference is tests/repetition_ref.py, checked against transformers' processors).  Both
// are defined over the hypothesis' GENERATED tokens seq[sample_begin : len] only (never the prompt):
//   repetition penalty p: every id in that history gets x < 0 ? x * p : x / p (timestamps included);
//   no-repeat n-gram n: every id that would complete an n-gram already in that history is masked.
// They live in their own instantiations (RULES): with both off the kernels launched are the ones without them.
//
// Sequence bias (BIAS; transformers' SequenceBiasLogitsProcessor over the same generated history): a table of
// (token sequence s_j, bias b_j), set per engine by wm_set_sequence_bias.  Entry j is active when the last n_j - 1
// generated tokens equal s_j[:-1] (n_j = 1: always), and every active entry adds b_j to the logit of s_j[-1].  The
// bias comes after the repetition penalty and before every mask (a masked id stays masked), so it feeds the timestamp
// forcing, the normaliser, the records and the beam candidates.  The engine stores the table sorted by the completing
// id (stable, so entries that end in one id keep their order): the entries of an id are one contiguous run, found by
// a binary search and summed in entry order, whatever the thread schedule.  A non-empty table selects the BIAS
// instantiations (which carry RULES); an empty one launches exactly the kernels above.
//
// Ragged prompts (RAG): one wm_generate call may hold windows whose prompts differ in length and whose total length
// limits differ.  The prompt length (p.sample_begin) and the limit (p.max_length) then come from per-hypothesis
// tables in device memory (p.hyp_begin / p.hyp_maxlen, indexed like seq_len), which the host fills once (lockstep
// decode) or hyp_start / beam_start fill when a slot takes a window (row-set decodes): kernel arguments never change,
// so captured step graphs stay valid across refills.  RAG is a template parameter of both select kernels: a call
// without the tables launches the same instantiations as before, unchanged.
//
// Per-window seeds (SEED): the Gumbel noise of a sampled call is keyed on (p.seed, global hypothesis row), so a
// window's draws depend on its place in the call.  With p.hyp_seed / p.hyp_key (per-hypothesis device tables, filled
// where hyp_begin / hyp_maxlen are) hypothesis h draws gumbel(hyp_seed[h], hyp_key[h], step, i): its window's own
// seed and its index among that window's hypotheses, which is what a call with the window alone and that seed draws.
// SEED is a template parameter of the MODE 2 instantiations only; without the tables a call launches what it
// launched before.
#include "search.h"
#include <stdexcept>
#include <string>

#define SB SEARCH_SB
#define NW (SB / 64)
#define KMAX 9

struct Cand { float v; int i; };
__device__ __forceinline__ bool better(float v1, int i1, float v2, int i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ float gumbel(unsigned long long seed, int hyp, int step, int i) {
  unsigned long long h = mix64(seed ^ mix64(((unsigned long long)hyp << 40) ^ ((unsigned long long)step << 20) ^ (unsigned long long)i));
  // 23 random bits: (k + 0.5) / 2^23 is exact in float32 and lies in (0, 1) for every k.  (With 24 bits, k = 2^24 - 1
  // rounded u up to exactly 1.0f and the key to +inf: that token was drawn with certainty, ~0.3 % of steps.)
  const float u = ((float)(h >> 41) + 0.5f) * (1.0f / 8388608.0f);
  return -logf(-logf(u));
}

// block-wide (max, argmax) reduce; returns result in all threads
__device__ Cand block_argmax(Cand c, Cand* sh) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(c.v, o, 64);
    const int i2 = __shfl_xor(c.i, o, 64);
    if (better(v2, i2, c.v, c.i)) { c.v = v2; c.i = i2; }
  }
  __syncthreads();
  if (lane == 0) sh[wv] = c;
  __syncthreads();
  Cand r = sh[0];
  for (int w = 1; w < NW; ++w)
    if (better(sh[w].v, sh[w].i, r.v, r.i)) r = sh[w];
  return r;
}
__device__ float block_sum(float v, float* sh) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  float r = 0.f;
  for (int w = 0; w < NW; ++w) r += sh[w];
  return r;
}

// MODE = p.mode as a template parameter (0 greedy, 1 beam top-k, 2 sampling): each instantiation only holds
// the registers its mode needs next to the register-resident row.
// REC: also write the per-step records (p.tok_lp / p.tok_lp_other; an extra register pass for the best other
// token), instantiated only when a caller asks for them.
// RULES: the repetition penalty / no-repeat n-gram rules (header comment).  Two LDS tables in the suppress_bits
// layout (id t -> word t % SB, bit t / SB) are filled by the history scan that already finds the last timestamp:
// s_seen marks the ids of the generated history, s_ban the ids an n-gram repeat would complete.  Each thread then
// reads its own two words once: the ban word joins `rule`, the seen word rescales the register-resident row.
// BIAS (with RULES): the sequence bias.  One thread per table entry compares the entry's prefix with the history tail
// and writes its bias (0 when inactive) to s_bval and, when active, the completing id's bit to s_bias (s_seen layout).
// A thread whose s_bias word is non-zero (rare) sums the id's run of entries and adds it to the register-resident row.
// SEED (MODE 2): the noise key comes from p.hyp_seed / p.hyp_key (header comment); h is block-uniform, so both are
// read once per block.
template <int MODE, bool REC, bool RULES, bool RAG, bool BIAS = false, bool SEED = false>
__global__ __launch_bounds__(SB) void logits_select_kernel(SearchParams p) {
  static_assert(!BIAS || RULES, "the sequence bias lives in the RULES instantiations");
  static_assert(!SEED || MODE == 2, "per-window seeds belong to sampling");
  __shared__ unsigned long long s_seen[RULES ? SB : 1];
  __shared__ unsigned long long s_ban[RULES ? SB : 1];
  __shared__ unsigned long long s_bias[BIAS ? SB : 1];
  __shared__ int s_bid[BIAS ? SEARCH_BIAS_MAX : 1];        // entry -> its completing id (ascending)
  __shared__ float s_bval[BIAS ? SEARCH_BIAS_MAX : 1];     // entry -> its bias if active at this step, else 0
  __shared__ Cand sh_c[NW];
  __shared__ float sh_f[NW];
  __shared__ int s_info[4];
  __shared__ Cand s_top[NW * KMAX];
  __shared__ int s_last_ts;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int h = p.row_hyp ? p.row_hyp[row] : row;
  if (p.done[h]) return;
  const int len = p.seq_len[h];
  const int sample_begin = RAG ? p.hyp_begin[h] : p.sample_begin;       // this hypothesis' prompt length
  const int* seq = p.tokens + (long long)h * p.n_ctx;
  const int tb = p.ts_begin;
  // position of the last sampled timestamp: a block-wide max instead of a serial backward scan (a text-only
  // history made thread 0 walk the whole sequence one dependent load at a time)
  if (tid == 0) s_last_ts = -1;
  if (RULES) {
    s_seen[tid] = 0;
    s_ban[tid] = 0;
  }
  if (BIAS) s_bias[tid] = 0;
  __syncthreads();
  if (BIAS) {
    const int G = len - sample_begin;
    for (int j = tid; j < p.n_bias; j += SB) {
      const int o0 = p.bias_off[j], nj = p.bias_off[j + 1] - o0;
      const int* sj = p.bias_tok + o0;
      const int t = sj[nj - 1];
      // the last nj - 1 generated tokens against s_j[:-1]: nj - 1 <= G keeps seq[len - m] inside the history
      bool act = nj - 1 <= G;
      for (int m = 1; m < nj && act; ++m) act = sj[nj - 1 - m] == seq[len - m];
      s_bid[j] = t;
      s_bval[j] = act ? p.bias_val[j] : 0.f;
      if (act) atomicOr((unsigned*)s_bias + 2 * (t % SB) + ((t / SB) >> 5), 1u << ((t / SB) & 31));
    }
  }
  for (int i = sample_begin + tid; i < len; i += SB) {
    const int t = seq[i];
    if (t >= tb) atomicMax(&s_last_ts, i);
    if (RULES && t >= 0 && t < SB * 64) {
      const int w = 2 * (t % SB) + ((t / SB) >> 5);        // 32-bit half of the id's 64-bit word
      const unsigned bit = 1u << ((t / SB) & 31);
      if (p.rep_penalty != 1.0f) atomicOr((unsigned*)s_seen + w, bit);
      // seq[i] ends an n-gram of the history whose first n-1 tokens are the last n-1 generated: it may not follow them
      // again.  j = this token's index among the generated ones: its n-gram starts at j - (n-1) >= 0 (so the history
      // holds >= n tokens and every index below stays inside it).  n = 1 compares nothing: every generated id is banned.
      const int n = p.no_repeat_ngram, j = i - sample_begin;
      if (n > 0 && j >= n - 1) {
        bool same = true;
        for (int m = 1; m < n && same; ++m) same = seq[i - m] == seq[len - m];
        if (same) atomicOr((unsigned*)s_ban + w, bit);
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int ns = len - sample_begin;
    const int last = ns >= 1 ? seq[len - 1] : -1;
    const int last_ts = ns >= 1 && last >= tb;
    const int pen_ts = ns < 2 || seq[len - 2] >= tb;
    const int lastv = s_last_ts >= 0 ? seq[s_last_ts] : -1;
    int bound = tb;                          // timestamps in [tb, bound) are masked
    if (lastv >= 0) bound = (last_ts && !pen_ts) ? lastv : lastv + 1;
    s_info[0] = ns == 0;
    s_info[1] = (last_ts && pen_ts) ? 1 : ((last_ts && !pen_ts) ? 2 : 0);
    s_info[2] = bound;
  }
  __syncthreads();
  const int first = s_info[0], pair_rule = s_info[1], bound = s_info[2];
  const float* lg = p.logits + (long long)row * p.ldl;
  const int V = p.V;
  const bool ts_on = p.with_ts != 0;
  const unsigned long long sup = p.suppress_bits[tid];
  // The rules as 64-bit masks over this thread's ids i = tid + k SB (bit k): every rule is a range or a single
  // id, so each costs O(1) instead of a branch chain per element (the per-element form was most of the
  // kernel's 11-17 k instructions of straight-line code)
  auto ge_mask = [&](long long x) -> unsigned long long {   // ids >= x
    const long long d = x - tid;
    if (d <= 0) return ~0ull;
    const long long k0 = (d + SB - 1) / SB;
    return k0 >= 64 ? 0ull : (~0ull << k0);
  };
  auto id_bit = [&](long long x) -> unsigned long long {    // the single id x
    const long long d = x - tid;
    return (d >= 0 && d % SB == 0 && d / SB < 64) ? (1ull << (d / SB)) : 0ull;
  };
  const unsigned long long ts_mask = ge_mask(tb);
  unsigned long long rule = 0;
  if (first && p.suppress_blank) rule |= id_bit(p.blank) | id_bit(p.eot);
  if (ts_on) {
    rule |= id_bit(p.no_timestamps);
    if (pair_rule == 1) rule |= ts_mask;
    rule |= ts_mask & ~ge_mask(bound);                                     // timestamps below the bound
    if (first && p.max_initial >= 0) rule |= ts_mask & ge_mask((long long)tb + p.max_initial + 1);
    if (pair_rule == 2) rule |= ~ts_mask & ~ge_mask(p.eot);                 // text below <|endoftext|>
    if (first) rule |= ~ts_mask;
  }
  // The row is loaded ONCE into registers (PER values per thread, every load issued before any is used),
  // masked entries recorded in a bitmask; both passes then run on registers.  (The earlier form looped
  // over the row twice with one dependent global load per iteration: ~90 us per launch of exposed latency.)
  // Beam (MODE 1) extracts its top-k in a third pass over the same registers, once `forced` is known.
  constexpr int PER = SEARCH_PER;                          // vocab <= 53248
  constexpr bool RES = true;
  float xv[RES ? PER : 1];
  unsigned long long live = 0;
  auto xat = [&](int k) -> float { return RES ? xv[k] : lg[tid + k * SB]; };
  if (RES) {
    // 32-bit byte offsets from the row base (global_load_dword v, v_off, s_base): one offset register per
    // load in flight instead of a 64-bit address each (that form spilled and waited on its spills), no
    // branches; ids >= V re-read the last id (never live: suppress_bits)
#pragma unroll
    for (int k = 0; k < PER; ++k)
      xv[RES ? k : 0] = *(const float*)((const char*)lg + (unsigned)(min(tid + k * SB, V - 1) * 4));
  }
  if (RULES) {
    rule |= s_ban[tid];
    const unsigned long long seen = s_seen[tid];
    const float pen = p.rep_penalty, inv_pen = 1.0f / pen;
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if ((seen >> k) & 1) xv[k] *= xv[k] < 0.f ? pen : inv_pen;
  }
  // the summed bias of id t: its run of entries starts at the lower bound of t in s_bid; inactive entries add 0
  auto bias_of = [&](int t) -> float {
    int lo = 0, hi = p.n_bias;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_bid[BIAS ? mid : 0] < t) lo = mid + 1; else hi = mid;
    }
    float add = 0.f;
    for (; lo < p.n_bias && s_bid[BIAS ? lo : 0] == t; ++lo) add += s_bval[BIAS ? lo : 0];
    return add;
  };
  if (BIAS) {
    // (a loop over the set bits with an unrolled select: xv is never indexed dynamically, and the search stands once)
    for (unsigned long long bw = s_bias[tid]; bw; bw &= bw - 1) {
      const int kb = __builtin_ctzll(bw);
      const float add = bias_of(tid + kb * SB);
#pragma unroll
      for (int k = 0; k < PER; ++k)
        if (k == kb) xv[k] += add;
    }
  }
  live = ~(sup | rule) & ((1ull << PER) - 1);
  // pass 1: per-segment max / argmax (and Gumbel keys for sampling, local top-k for beam)
  Cand mt{-INFINITY, 0x7fffffff}, ms{-INFINITY, 0x7fffffff};
  Cand gt{-INFINITY, 0x7fffffff}, gs{-INFINITY, 0x7fffffff};
  const int K = MODE == 1 ? p.topk : 0;
  // Gumbel noise keyed on the WINDOW's hypothesis id, not the slot: the row-set decode reuses slots, and a window's
  // draws must not depend on which slot it got (hyp_out[h] = w there, one hypothesis per window; h = w*nh + j else)
  // SEED: the window's own seed and the hypothesis' index inside its window, whatever slot or place it has
  const int gkey = SEED ? p.hyp_key[h] : (MODE == 2 && p.hyp_out ? p.hyp_out[h] : h);
  const unsigned long long gseed = SEED ? p.hyp_seed[h] : p.seed;
  // (explicit branches, not a reference chosen per element: a `Cand& m = is_ts ? ms : mt` put both in scratch;
  // a select-only form of this pass spilled)
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (!((live >> k) & 1)) continue;
    const int i = tid + k * SB;
    const float x = xat(k);
    const bool is_ts = (ts_mask >> k) & 1;
    if (is_ts) {
      if (better(x, i, ms.v, ms.i)) { ms.v = x; ms.i = i; }
    } else {
      if (better(x, i, mt.v, mt.i)) { mt.v = x; mt.i = i; }
    }
    if (MODE == 2) {
      // the decode step of this hypothesis = tokens it has sampled so far (equal to the host's step counter
      // for every live hypothesis; read from the device so a captured step graph replays unchanged)
      const float key = x * p.inv_temperature + gumbel(gseed, gkey, len - sample_begin, i);
      if (is_ts) {
        if (better(key, i, gs.v, gs.i)) { gs.v = key; gs.i = i; }
      } else {
        if (better(key, i, gt.v, gt.i)) { gt.v = key; gt.i = i; }
      }
    }
  }
  mt = block_argmax(mt, sh_c);
  ms = block_argmax(ms, sh_c);
  // pass 2: sum-exp per segment
  float st = 0.f, ss = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (!((live >> k) & 1)) continue;
    if ((ts_mask >> k) & 1) ss += expf(xat(k) - ms.v);
    else st += expf(xat(k) - mt.v);
  }
  st = block_sum(st, sh_f);
  ss = block_sum(ss, sh_f);
  // Numeric breakage is an error, never a token: a NaN or +inf among the allowed logits makes its segment's
  // exp-sum NaN (NaN, and inf - inf, propagate through the sums), and a row whose rules allow nothing leaves both
  // maxima at -inf.  The hypothesis ends, the device error word records it, and the host raises at its next poll
  // (the worker turns that into FAILED, worker/transcription.py:436-443).  All tested values are block-uniform.
  if (isnan(st) || isnan(ss) || (mt.v == -INFINITY && ms.v == -INFINITY)) {
    if (tid == 0) {
      wm_report_error(p.err, (isnan(st) || isnan(ss)) ? WM_ERR_NONFINITE : WM_ERR_NO_TOKEN, h, len - sample_begin);
      if (MODE == 1) {
        for (int r = 0; r < p.topk; ++r) {
          p.cand_tok[(long long)h * p.topk + r] = -1;
          p.cand_lp[(long long)h * p.topk + r] = -INFINITY;
        }
      } else {
        p.done[h] = 1;
        atomicSub(p.n_active, 1);
      }
    }
    return;
  }
  const float lse_t = mt.v > -INFINITY ? mt.v + logf(st) : -INFINITY;
  const float lse_s = ms.v > -INFINITY ? ms.v + logf(ss) : -INFINITY;
  const bool forced = ts_on && lse_s > mt.v;
  float Z;
  if (forced) Z = lse_s;
  else if (lse_t == -INFINITY) Z = lse_s;
  else if (lse_s == -INFINITY) Z = lse_t;
  else Z = fmaxf(lse_t, lse_s) + log1pf(expf(-fabsf(lse_t - lse_s)));

  if (MODE == 1) {
    // pass 3: the top-K of the allowed set (timestamps only when forced), in `better` order.  A threshold
    // first: tau = the K-th best of the per-thread maxima (K distinct elements are >= tau, so every top-K
    // element is too); the few elements >= tau are appended to an LDS list and wave 0 ranks them.  (The
    // earlier form ran K rounds of a wave argmax over the whole register-resident row: K x 52 compare-selects
    // per thread, ~79 us per launch at beam 5, one CU per hypothesis.)  A list that overflows (ties) falls
    // back to that form, so the result is the exact top-K either way.
    unsigned long long avail = live;
    if (forced) avail &= ts_mask;
    const int wv = tid >> 6, lane = tid & 63;
    constexpr int LCAP = 256;
    __shared__ Cand s_list[LCAP];
    __shared__ int s_n;
    __shared__ Cand s_tau;
    {
      Cand lb{-INFINITY, 0x7fffffff};        // this thread's best allowed element
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int i = tid + k * SB;
        if (((avail >> k) & 1) && better(xat(k), i, lb.v, lb.i)) { lb.v = xat(k); lb.i = i; }
      }
      for (int r = 0; r < K; ++r) {          // the wave's K best per-thread maxima
        Cand best = lb;
        int owner = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float v2 = __shfl_xor(best.v, o, 64);
          const int i2 = __shfl_xor(best.i, o, 64);
          const int ow2 = __shfl_xor(owner, o, 64);
          if (better(v2, i2, best.v, best.i) || (v2 == best.v && i2 == best.i && ow2 < owner)) {
            best.v = v2; best.i = i2; owner = ow2;
          }
        }
        if (lane == 0) s_top[wv * KMAX + r] = best;
        if (lane == owner) lb = Cand{-INFINITY, 0x7fffffff};
      }
    }
    __shared__ int s_ptr[NW];
    if (tid < NW) s_ptr[tid] = 0;
    if (tid == 0) s_n = 0;
    __syncthreads();
    if (tid == 0) {                          // tau: the K-th of the merged per-wave lists
      Cand tau{-INFINITY, 0x7fffffff};
      for (int r = 0; r < K; ++r) {
        Cand best{-INFINITY, 0x7fffffff};
        int bw = -1;
        for (int w = 0; w < NW; ++w) {
          const int pp = s_ptr[w];
          if (pp >= K) continue;
          const Cand c = s_top[w * KMAX + pp];
          if (better(c.v, c.i, best.v, best.i)) { best = c; bw = w; }
        }
        if (bw < 0) { tau = Cand{-INFINITY, 0x7fffffff}; break; }
        ++s_ptr[bw];
        tau = best;
      }
      s_tau = tau;
    }
    __syncthreads();
    const Cand tau = s_tau;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * SB;
      if (((avail >> k) & 1) && (better(xat(k), i, tau.v, tau.i) || (xat(k) == tau.v && i == tau.i))) {
        const int at = atomicAdd(&s_n, 1);
        if (at < LCAP) s_list[at] = Cand{xat(k), i};
      }
    }
    __syncthreads();
    const int n_list = s_n;
    if (n_list <= LCAP && !(p.abl & 2)) {
      if (wv == 0) {
        Cand c[LCAP / 64];
#pragma unroll
        for (int j = 0; j < LCAP / 64; ++j)
          c[j] = lane + 64 * j < n_list ? s_list[lane + 64 * j] : Cand{-INFINITY, 0x7fffffff};
        for (int r = 0; r < K; ++r) {
          Cand best = c[0];
          int bj = 0;
#pragma unroll
          for (int j = 1; j < LCAP / 64; ++j)
            if (better(c[j].v, c[j].i, best.v, best.i)) { best = c[j]; bj = j; }
          int owner = lane;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(best.v, o, 64);
            const int i2 = __shfl_xor(best.i, o, 64);
            const int ow2 = __shfl_xor(owner, o, 64);
            if (better(v2, i2, best.v, best.i) || (v2 == best.v && i2 == best.i && ow2 < owner)) {
              best.v = v2; best.i = i2; owner = ow2;
            }
          }
          if (lane == owner) {
#pragma unroll
            for (int j = 0; j < LCAP / 64; ++j)
              if (j == bj) c[j] = Cand{-INFINITY, 0x7fffffff};
          }
          if (lane == 0) {
            const bool none = best.v == -INFINITY;
            p.cand_tok[(long long)h * p.topk + r] = none ? -1 : best.i;
            p.cand_lp[(long long)h * p.topk + r] = none ? -INFINITY : best.v - Z;
          }
        }
      }
      return;
    }
    // overflow (many tied values): K rounds over the whole row
    for (int r = 0; r < K; ++r) {
      Cand best{-INFINITY, 0x7fffffff};
      int bk = -1;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int i = tid + k * SB;
        if (((avail >> k) & 1) && better(xat(k), i, best.v, best.i)) { best.v = xat(k); best.i = i; bk = k; }
      }
      int owner = lane;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(best.v, o, 64);
        const int i2 = __shfl_xor(best.i, o, 64);
        const int ow2 = __shfl_xor(owner, o, 64);
        if (better(v2, i2, best.v, best.i) || (v2 == best.v && i2 == best.i && ow2 < owner)) {
          best.v = v2; best.i = i2; owner = ow2;
        }
      }
      if (lane == 0) s_top[wv * KMAX + r] = best;
      if (lane == owner && bk >= 0) avail &= ~(1ull << bk);
    }
    if (tid < NW) s_ptr[tid] = 0;
    __syncthreads();
    if (tid == 0) {
      for (int r = 0; r < K; ++r) {
        Cand best{-INFINITY, 0x7fffffff};
        int bw = -1;
        for (int w = 0; w < NW; ++w) {
          const int pp = s_ptr[w];
          if (pp >= K) continue;
          const Cand c = s_top[w * KMAX + pp];
          if (better(c.v, c.i, best.v, best.i)) { best = c; bw = w; }
        }
        if (bw < 0 || best.v == -INFINITY) {
          p.cand_tok[(long long)h * p.topk + r] = -1;
          p.cand_lp[(long long)h * p.topk + r] = -INFINITY;
        } else {
          ++s_ptr[bw];
          p.cand_tok[(long long)h * p.topk + r] = best.i;
          p.cand_lp[(long long)h * p.topk + r] = best.v - Z;
        }
      }
    }
    return;
  }

  if (MODE == 2) {
    gt = block_argmax(gt, sh_c);
    gs = block_argmax(gs, sh_c);
  }
  // the chosen token: every thread holds the block-reduced candidates and `forced`, so it is block-uniform
  int tok;
  if (MODE == 2) tok = forced ? gs.i : (better(gt.v, gt.i, gs.v, gs.i) ? gt.i : gs.i);
  else tok = forced ? ms.i : (better(mt.v, mt.i, ms.v, ms.i) ? mt.i : ms.i);
  float lp_other = -INFINITY;
  if (REC) {
    // the best allowed token other than the chosen one (the per-step margin of the records)
    const unsigned long long avail = forced ? (live & ts_mask) : live;
    Cand b{-INFINITY, 0x7fffffff};
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * SB;
      if (((avail >> k) & 1) && i != tok && better(xat(k), i, b.v, b.i)) { b.v = xat(k); b.i = i; }
    }
    b = block_argmax(b, sh_c);
    lp_other = b.v - Z;
  }
  __shared__ int s_fin;
  if (tid == 0) {
    // (the row's registers belong to another thread: re-read the logit and, RULES, penalise it exactly as above)
    float lp;
    if constexpr (RULES) {
      float xt = lg[tok];
      if ((s_seen[tok % SB] >> (tok / SB)) & 1) xt *= xt < 0.f ? p.rep_penalty : 1.0f / p.rep_penalty;
      if constexpr (BIAS) {
        if ((s_bias[tok % SB] >> (tok / SB)) & 1) xt += bias_of(tok);
      }
      lp = xt - Z;
    } else {
      lp = lg[tok] - Z;
    }
    const float cum = p.cum[h] + lp;
    p.cum[h] = cum;
    if (REC && p.tok_lp) {
      p.tok_lp[(long long)h * p.n_ctx + len] = lp;
      if (p.tok_lp_other) p.tok_lp_other[(long long)h * p.n_ctx + len] = lp_other;
    }
    bool fin = false;
    if (tok == p.eot) {
      fin = true;
    } else {
      p.tokens[(long long)h * p.n_ctx + len] = tok;
      p.seq_len[h] = len + 1;
      p.row_tok[row] = tok;
      p.row_pos[row] = len;
      if (len + 1 >= (RAG ? p.hyp_maxlen[h] : p.max_length)) fin = true;
    }
    if (fin) {
      p.done[h] = 1;
      atomicSub(p.n_active, 1);
      if (p.res_tok) {
        const int o = p.hyp_out[h];
        p.res_len[o] = len + (tok == p.eot ? 0 : 1) - sample_begin;
        p.res_cum[o] = cum;
      }
    }
    s_fin = fin;
  }
  if (p.res_tok) {
    // row-set decode: the hypothesis' slot is reused once it ends, so its tokens (and records) move to the
    // output tables now, copied by the whole block
    __syncthreads();
    if (s_fin) {
      const int o = p.hyp_out[h];
      const int n = len + (tok == p.eot ? 0 : 1) - sample_begin;     // generated tokens, <|endoftext|> excluded
      const int* src = p.tokens + (long long)h * p.n_ctx + sample_begin;
      for (int t = tid; t < n; t += SB) p.res_tok[(long long)o * p.n_ctx + t] = src[t];
      if (REC && p.tok_lp && p.res_lp) {
        const int nr = len + 1 - sample_begin;                       // records up to position len
        const float* a = p.tok_lp + (long long)h * p.n_ctx + sample_begin;
        const float* b = p.tok_lp_other ? p.tok_lp_other + (long long)h * p.n_ctx + sample_begin : nullptr;
        for (int t = tid; t < nr; t += SB) {
          p.res_lp[(long long)o * p.n_ctx + t] = a[t];
          if (b && p.res_lp_other) p.res_lp_other[(long long)o * p.n_ctx + t] = b[t];
        }
      }
    }
  }
}

void search_suppress_bits(const unsigned char* sup, int V, unsigned long long* bits) {
  for (int t = 0; t < SB; ++t) {
    unsigned long long w = 0;
    for (int k = 0; k < 64; ++k) {
      const long long i = t + (long long)k * SB;
      if (i >= V || sup[i]) w |= 1ull << k;
    }
    bits[t] = w;
  }
}

void launch_logits_select(const SearchParams& p, int n_rows, hipStream_t st) {
  if (n_rows <= 0) return;
  if (p.V > 53248) throw std::runtime_error("logits_select: vocabulary larger than 53248");
  if (p.mode == 1 && (p.topk < 1 || p.topk > KMAX)) throw std::runtime_error("beam size must be <= 8");
  if (p.res_tok && (!p.hyp_out || !p.res_len || !p.res_cum || p.mode == 1))
    throw std::runtime_error("logits_select: incomplete output tables");
  const bool rec = p.tok_lp != nullptr && p.mode != 1;     // beam: beam_select_kernel keeps the records
  if (!(p.rep_penalty > 0.f) || p.no_repeat_ngram < 0)
    throw std::runtime_error("logits_select: repetition penalty must be > 0 and the n-gram size >= 0");
  if (p.n_bias < 0 || p.n_bias > SEARCH_BIAS_MAX || (p.n_bias > 0 && (!p.bias_off || !p.bias_tok || !p.bias_val)))
    throw std::runtime_error("logits_select: bad sequence-bias table");
  const bool bias = p.n_bias > 0;
  const bool rules = bias || p.rep_penalty != 1.0f || p.no_repeat_ngram > 0;
  if ((p.hyp_begin != nullptr) != (p.hyp_maxlen != nullptr))
    throw std::runtime_error("logits_select: the per-hypothesis tables come as a pair");
  const bool rag = p.hyp_begin != nullptr;
  if ((p.hyp_seed != nullptr) != (p.hyp_key != nullptr))
    throw std::runtime_error("logits_select: the per-hypothesis seed tables come as a pair");
  if (p.hyp_seed && p.mode != 2) throw std::runtime_error("logits_select: per-window seeds need sampling");
  const bool seeded = p.hyp_seed != nullptr;
  const dim3 g(n_rows), b(SB);
#define SEL_LAUNCH(MODE, REC, RULES)                                                                      \
  do {                                                                                                    \
    if (RULES && bias) {                                                                                  \
      if (rag) hipLaunchKernelGGL((logits_select_kernel<MODE, REC, true, true, true>), g, b, 0, st, p);   \
      else hipLaunchKernelGGL((logits_select_kernel<MODE, REC, true, false, true>), g, b, 0, st, p);      \
    } else if (rag) {                                                                                     \
      hipLaunchKernelGGL((logits_select_kernel<MODE, REC, RULES, true>), g, b, 0, st, p);                 \
    } else {                                                                                              \
      hipLaunchKernelGGL((logits_select_kernel<MODE, REC, RULES, false>), g, b, 0, st, p);                \
    }                                                                                                     \
  } while (0)
  // sampling: the same choice, and with per-window seeds the SEED instantiations
#define SEL_LAUNCH_S(REC, RULES)                                                                               \
  do {                                                                                                         \
    if (!seeded) {                                                                                             \
      SEL_LAUNCH(2, REC, RULES);                                                                               \
    } else if (RULES && bias) {                                                                                \
      if (rag) hipLaunchKernelGGL((logits_select_kernel<2, REC, true, true, true, true>), g, b, 0, st, p);     \
      else hipLaunchKernelGGL((logits_select_kernel<2, REC, true, false, true, true>), g, b, 0, st, p);        \
    } else if (rag) {                                                                                          \
      hipLaunchKernelGGL((logits_select_kernel<2, REC, RULES, true, false, true>), g, b, 0, st, p);            \
    } else {                                                                                                   \
      hipLaunchKernelGGL((logits_select_kernel<2, REC, RULES, false, false, true>), g, b, 0, st, p);           \
    }                                                                                                          \
  } while (0)
  switch ((rules ? 6 : 0) + p.mode * 2 + (rec ? 1 : 0)) {
    case 0: SEL_LAUNCH(0, false, false); break;
    case 1: SEL_LAUNCH(0, true, false); break;
    case 2: case 3: SEL_LAUNCH(1, false, false); break;
    case 4: SEL_LAUNCH_S(false, false); break;
    case 5: SEL_LAUNCH_S(true, false); break;
    case 6: SEL_LAUNCH(0, false, true); break;
    case 7: SEL_LAUNCH(0, true, true); break;
    case 8: case 9: SEL_LAUNCH(1, false, true); break;
    case 10: SEL_LAUNCH_S(false, true); break;
    default: SEL_LAUNCH_S(true, true); break;
  }
#undef SEL_LAUNCH_S
#undef SEL_LAUNCH
  WM_LAUNCH_CHECK("logits_select_kernel");
}

// ------------------------------------------------------------------------------------ row-set bookkeeping
__global__ __launch_bounds__(256) void hyp_start_kernel(const int* __restrict__ hs, const int* __restrict__ ws,
                                                        const int* __restrict__ win_prompt, int P,
                                                        const int* __restrict__ win_slot, int n_ctx, int* tokens,
                                                        int* seq_len, int* done, float* cum, int* hyp_slot, int* hyp_out,
                                                        const int* __restrict__ win_len,
                                                        const int* __restrict__ win_maxlen, int* hyp_begin,
                                                        int* hyp_maxlen,
                                                        const unsigned long long* __restrict__ win_seed,
                                                        unsigned long long* hyp_seed, int* hyp_key) {
  const int h = hs[blockIdx.x], w = ws[blockIdx.x];
  // ragged prompts: P is the row stride of win_prompt, the window's own length comes from win_len (the padding
  // behind it is not read) and the slot's rows of the selection tables are filled here
  const int n = win_len ? win_len[w] : P;
  for (int p = threadIdx.x; p < n; p += blockDim.x) tokens[(long long)h * n_ctx + p] = win_prompt[(long long)w * P + p];
  if (threadIdx.x == 0) {
    if (win_len) {
      hyp_begin[h] = n;
      hyp_maxlen[h] = win_maxlen[w];
    }
    if (win_seed) {                            // per-window seeds: the slot draws as its window's hypothesis 0
      hyp_seed[h] = win_seed[w];
      hyp_key[h] = 0;
    }
    seq_len[h] = n;
    done[h] = 0;
    cum[h] = 0.f;
    hyp_slot[h] = win_slot[w];
    hyp_out[h] = w;
  }
}

void launch_hyp_start(int n, const int* hs, const int* ws, const int* win_prompt, int P, const int* win_slot, int n_ctx,
                      int* tokens, int* seq_len, int* done, float* cum, int* hyp_slot, int* hyp_out, hipStream_t st,
                      const int* win_len, const int* win_maxlen, int* hyp_begin, int* hyp_maxlen,
                      const unsigned long long* win_seed, unsigned long long* hyp_seed, int* hyp_key) {
  if (n <= 0) return;
  if (win_len && (!win_maxlen || !hyp_begin || !hyp_maxlen)) throw std::runtime_error("hyp_start: incomplete ragged tables");
  if (win_seed && (!hyp_seed || !hyp_key)) throw std::runtime_error("hyp_start: incomplete seed tables");
  hipLaunchKernelGGL(hyp_start_kernel, dim3(n), dim3(64), 0, st, hs, ws, win_prompt, P, win_slot, n_ctx, tokens, seq_len,
                     done, cum, hyp_slot, hyp_out, win_len, win_maxlen, hyp_begin, hyp_maxlen, win_seed, hyp_seed, hyp_key);
  WM_LAUNCH_CHECK("hyp_start_kernel");
}

// Beam row-set decode: group gs[i] of K hypothesis slots starts window ws[i]: every hypothesis gets the window's
// prompt, its lineage points the prompt positions at the group's first slot (whose self-KV the pass prefills), the
// first slot carries the score (the others start dead, as the one-pass beam prefill), and the group's finished list
// is emptied.
__global__ __launch_bounds__(256) void beam_start_kernel(const int* __restrict__ gs, const int* __restrict__ ws, int K,
                                                         const int* __restrict__ win_prompt, int P,
                                                         const int* __restrict__ win_slot, int n_ctx, int* tokens,
                                                         int* lin, int* seq_len, int* done, float* cum, int* hyp_slot,
                                                         int* n_fin, const int* __restrict__ win_len,
                                                         const int* __restrict__ win_maxlen, int* hyp_begin,
                                                         int* hyp_maxlen) {
  const int g = gs[blockIdx.x], w = ws[blockIdx.x], h0 = g * K;
  const int n = win_len ? win_len[w] : P;      // ragged prompts: as hyp_start_kernel
  for (int i = threadIdx.x; i < K * n; i += blockDim.x) {
    const int b = i / n, p = i - b * n;
    tokens[(long long)(h0 + b) * n_ctx + p] = win_prompt[(long long)w * P + p];
    lin[(long long)(h0 + b) * n_ctx + p] = h0;
  }
  if (threadIdx.x < K) {
    const int h = h0 + threadIdx.x;
    if (win_len) {
      hyp_begin[h] = n;
      hyp_maxlen[h] = win_maxlen[w];
    }
    seq_len[h] = n;
    done[h] = 0;
    cum[h] = threadIdx.x == 0 ? 0.f : -INFINITY;
    hyp_slot[h] = win_slot[w];
  }
  if (threadIdx.x == 0) n_fin[g] = 0;
}

void launch_beam_start(int n, const int* gs, const int* ws, int K, const int* win_prompt, int P, const int* win_slot,
                       int n_ctx, int* tokens, int* lin, int* seq_len, int* done, float* cum, int* hyp_slot, int* n_fin,
                       hipStream_t st, const int* win_len, const int* win_maxlen, int* hyp_begin, int* hyp_maxlen) {
  if (n <= 0) return;
  if (win_len && (!win_maxlen || !hyp_begin || !hyp_maxlen)) throw std::runtime_error("beam_start: incomplete ragged tables");
  hipLaunchKernelGGL(beam_start_kernel, dim3(n), dim3(256), 0, st, gs, ws, K, win_prompt, P, win_slot, n_ctx, tokens,
                     lin, seq_len, done, cum, hyp_slot, n_fin, win_len, win_maxlen, hyp_begin, hyp_maxlen);
  WM_LAUNCH_CHECK("beam_start_kernel");
}

__global__ __launch_bounds__(256) void rows_fill_kernel(int n, const int* __restrict__ src, int* __restrict__ tok,
                                                        int* __restrict__ pos, const int* __restrict__ row_tok,
                                                        const int* __restrict__ row_pos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = src[i];
  if (s >= 0) {
    tok[i] = row_tok[s];
    pos[i] = row_pos[s];
  }
}

void launch_rows_fill(int n, const int* src, int* tok, int* pos, const int* row_tok, const int* row_pos, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(rows_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, src, tok, pos, row_tok, row_pos);
  WM_LAUNCH_CHECK("rows_fill_kernel");
}

__global__ __launch_bounds__(256) void rows_scatter_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           const int* __restrict__ dst_row, int V) {
  const float* s = src + (long long)blockIdx.x * V;
  float* d = dst + (long long)dst_row[blockIdx.x] * V;
  for (int i = threadIdx.x; i < V; i += blockDim.x) d[i] = s[i];
}

void launch_rows_scatter(const float* src, float* dst, const int* dst_row, int n, int V, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(rows_scatter_kernel, dim3(n), dim3(256), 0, st, src, dst, dst_row, V);
  WM_LAUNCH_CHECK("rows_scatter_kernel");
}

// ------------------------------------------------------------------------------------ beam bookkeeping
#define BMAX 8
#define CMAX 16

// One workgroup per window.  The K x (K+1) candidates are ranked in parallel (rank = number of candidates
// that precede it in a stable descending sort of (beam, rank)-ordered candidates), and the ranked list lives in
// LDS, so the one serial walk (live beams / finished list, <= K (K+1) steps) touches no scratch memory; the
// finished hypotheses' tokens are copied by the whole workgroup.  (The earlier form ran an insertion sort and
// the copies in thread 0 over scratch arrays: ~0.2 ms per decode step of the sequential beam-5 call.)
template <bool RAG>
__global__ __launch_bounds__(256) void beam_select_kernel(BeamParams p) {
  constexpr int NC = BMAX * (BMAX + 1);
  __shared__ int s_tok[BMAX][448];
  __shared__ int s_lin[BMAX][448];
  __shared__ float s_lp[BMAX][448];          // per-step records (p.tok_lp)
  __shared__ float c_sc[NC], o_sc[NC];
  __shared__ int c_ok[NC], o_src[NC], o_tk[NC];
  __shared__ int s_par[BMAX], s_new[BMAX];
  __shared__ float s_sc[BMAX], s_cum[BMAX];
  __shared__ int f_src[CMAX], f_slot[CMAX];
  __shared__ float f_sc[CMAX];
  __shared__ int s_nlive, s_nf_new;
  const int w = blockIdx.x, tid = threadIdx.x;
  const int K = p.beam, h0 = w * K, T = K + 1, NK = K * T;
  if (p.done[h0]) return;
  const int len = p.seq_len[h0];
  // the window's prompt length and length limit (RAG: from its first hypothesis' rows of the tables)
  const int sample_begin = RAG ? p.hyp_begin[h0] : p.sample_begin;
  const int max_length = RAG ? p.hyp_maxlen[h0] : p.max_length;
  const bool rec = p.tok_lp != nullptr;
  for (int i = tid; i < K * len; i += blockDim.x) {
    const int b = i / len, t = i - b * len;
    s_tok[b][t] = p.tokens[(long long)(h0 + b) * p.n_ctx + t];
    s_lin[b][t] = p.lin[(long long)(h0 + b) * p.n_ctx + t];
    if (rec) s_lp[b][t] = p.tok_lp[(long long)(h0 + b) * p.n_ctx + t];
  }
  // candidate i = (beam j, rank r) in (beam, rank) order
  float sc_i = -INFINITY;
  int tk_i = -1;
  if (tid < NK) {
    const int j = tid / T;
    const float c = p.cum[h0 + j];
    if (tid % T == 0) s_cum[j] = c;
    tk_i = p.cand_tok[(long long)h0 * T + tid];
    const float s = c + p.cand_lp[(long long)h0 * T + tid];
    // a NaN score would compare false against every other and break the ranks' total order (the select kernel
    // already reports non-finite rows and emits no candidate for them; this keeps the ranking well-formed)
    const bool ok = c != -INFINITY && tk_i >= 0 && !isnan(s);
    if (ok) sc_i = s;
    c_ok[tid] = ok;
    c_sc[tid] = sc_i;
  }
  __syncthreads();
  if (tid < NK && c_ok[tid]) {
    int rank = 0;
    for (int j = 0; j < NK; ++j)
      if (c_ok[j] && (c_sc[j] > sc_i || (c_sc[j] == sc_i && j < tid))) ++rank;
    o_sc[rank] = sc_i; o_src[rank] = tid / T; o_tk[rank] = tk_i;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int j = 0; j < NK; ++j) n += c_ok[j];
    int nlive = 0, nf = p.n_fin[w], nnew = 0;
    for (int c = 0; c < n && nlive < K; ++c) {
      if (o_tk[c] == p.eot) {
        if (nf < p.max_cand) {
          f_src[nnew] = o_src[c]; f_slot[nnew] = nf; f_sc[nnew] = o_sc[c];
          ++nnew;
          ++nf;
        }
      } else {
        s_par[nlive] = o_src[c]; s_new[nlive] = o_tk[c]; s_sc[nlive] = o_sc[c]; ++nlive;
      }
    }
    if (nlive == 0) {
      // no live candidate (every candidate non-finite or finished): the dead beams below copy beam 0's lineage and a
      // valid token, so no later pass reads a hypothesis index or token from uninitialised LDS
      s_par[0] = 0; s_new[0] = p.eot; s_sc[0] = -INFINITY;
    }
    p.n_fin[w] = nf;
    s_nlive = nlive;
    s_nf_new = nnew;
    const bool fin = nf >= p.max_cand || len + 1 >= max_length || nlive == 0;
    if (fin) {
      for (int j = 0; j < K; ++j) p.done[h0 + j] = 1;
      atomicSub(p.n_active, K);
    }
  }
  __syncthreads();
  {
    const int nnew = s_nf_new, ng = len - sample_begin;
    for (int i = tid; i < nnew * ng; i += blockDim.x) {
      const int f = i / ng, t = i - f * ng;
      p.fin_tok[((long long)w * p.max_cand + f_slot[f]) * p.n_ctx + t] = s_tok[f_src[f]][sample_begin + t];
      if (rec) p.fin_lp[((long long)w * p.max_cand + f_slot[f]) * p.n_ctx + t] = s_lp[f_src[f]][sample_begin + t];
    }
    if (tid < nnew) {
      p.fin_len[w * p.max_cand + f_slot[tid]] = ng;
      p.fin_cum[w * p.max_cand + f_slot[tid]] = f_sc[tid];
      if (rec) p.fin_lp[((long long)w * p.max_cand + f_slot[tid]) * p.n_ctx + ng] = f_sc[tid] - s_cum[f_src[tid]];
    }
  }
  const int nlive = s_nlive;
  // write the new beams (beams beyond nlive are marked dead with cum = -inf)
  for (int i = tid; i < K * len; i += blockDim.x) {
    const int b = i / len, t = i - b * len;
    const int par = b < nlive ? s_par[b] : s_par[0];
    p.tokens[(long long)(h0 + b) * p.n_ctx + t] = s_tok[par][t];
    p.lin[(long long)(h0 + b) * p.n_ctx + t] = s_lin[par][t];
    if (rec) p.tok_lp[(long long)(h0 + b) * p.n_ctx + t] = s_lp[par][t];
  }
  __syncthreads();
  if (tid < K) {
    const int b = tid;
    const int par = b < nlive ? s_par[b] : s_par[0];
    const int tok = b < nlive ? s_new[b] : s_new[0];
    if (rec) p.tok_lp[(long long)(h0 + b) * p.n_ctx + len] = b < nlive ? s_sc[b] - s_cum[par] : -INFINITY;
    p.tokens[(long long)(h0 + b) * p.n_ctx + len] = tok;
    p.lin[(long long)(h0 + b) * p.n_ctx + len] = h0 + b;      // the next step writes KV at (hyp, len)
    p.seq_len[h0 + b] = len + 1;
    p.cum[h0 + b] = b < nlive ? s_sc[b] : -INFINITY;
    p.row_tok[h0 + b] = tok;
    p.row_pos[h0 + b] = len;
    (void)par;
  }
}

void launch_beam_select(const BeamParams& p, int n_win, hipStream_t st) {
  if (n_win <= 0) return;
  if (p.beam > BMAX || p.max_cand > CMAX || p.n_ctx > 448) throw std::runtime_error("beam_select: limits exceeded");
  if ((p.hyp_begin != nullptr) != (p.hyp_maxlen != nullptr))
    throw std::runtime_error("beam_select: the per-hypothesis tables come as a pair");
  if (p.hyp_begin) hipLaunchKernelGGL(beam_select_kernel<true>, dim3(n_win), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(beam_select_kernel<false>, dim3(n_win), dim3(256), 0, st, p);
  WM_LAUNCH_CHECK("beam_select_kernel");
}

// Language detection: out[r][j] = softmax over logits[r][lang_begin .. lang_begin + n_langs) (ctranslate2
// Whisper.detect_language's probabilities [FW↑]), f32 with an f32 max / sum
__global__ __launch_bounds__(256) void lang_probs_kernel(const float* __restrict__ logits, long long ldl, int lang_begin,
                                                         int n_langs, float* __restrict__ out) {
  __shared__ float sh[4];
  const float* lg = logits + (long long)blockIdx.x * ldl + lang_begin;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float m = -INFINITY;
  for (int j = tid; j < n_langs; j += 256) m = fmaxf(m, lg[j]);
  m = wave_max(m);
  if (lane == 0) sh[wv] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  float s = 0.f;
  for (int j = tid; j < n_langs; j += 256) s += expf(lg[j] - m);
  s = wave_sum(s);
  if (lane == 0) sh[wv] = s;
  __syncthreads();
  s = sh[0] + sh[1] + sh[2] + sh[3];
  for (int j = tid; j < n_langs; j += 256) out[(long long)blockIdx.x * n_langs + j] = expf(lg[j] - m) / s;
}

void launch_lang_probs(const float* logits, long long ldl, int rows, int lang_begin, int n_langs, float* out, hipStream_t st) {
  if (rows <= 0 || n_langs <= 0) return;
  hipLaunchKernelGGL(lang_probs_kernel, dim3(rows), dim3(256), 0, st, logits, ldl, lang_begin, n_langs, out);
  WM_LAUNCH_CHECK("lang_probs_kernel");
}

// Language head (wm_language_id): the language tokens' probabilities straight from the decoder's last hidden state,
// without the full-vocabulary logits.  One 256-thread workgroup per row, fused:
//   1. the final LayerNorm (dec.ln) in f32 with layernorm_kernel's statistics (norm.hip: one wave, lane l owns the
//      float2 pairs l + 64 i, the same sums in the same order; each of the four waves repeats them, so no block-wide
//      step is needed), rounded to bf16 as the logits GEMM's operand is, into LDS;
//   2. the dot products with rows lang_begin .. lang_begin + n_langs - 1 of the tied embedding: wave w takes languages
//      w, w + 4, ...; a lane owns the 16-B chunks lane + 64 s of a row (NS = ceil(D / 512) of them; D = 384 leaves lanes
//      48..63 idle, D = 1280 lanes 32..63 of the last step) and keeps its chunks of the normalised state in registers.
//      The loads of LB languages are issued together before the first use (NS * LB 16-B loads in flight per lane), then
//      each language's partial is summed over the wave.  Every product bf16 x bf16 is exact in f32, so the logit is an
//      f32 sum of the products the full-vocabulary GEMM sums, in another order;
//   3. the allowed mask (allowed[j] == 0: logit -inf, probability exactly 0); an allowed logit that is not finite
//      counts as masked, and a row that keeps no language is an error (err: WM_ERR_NONFINITE, the row);
//   4. the f32 softmax of lang_probs_kernel (f32 max and sum over the block, expf(x - max) / sum);
//   5. the argmax, the lowest index winning ties (block_argmax's rule).
// Nothing in a row's arithmetic depends on the other rows or on the grid.
#define LANG_MAX SEARCH_LANG_MAX
#define LANG_LB 8               // languages whose loads a wave issues together
// block_argmax for a 256-thread block (four waves): the same rule and order
__device__ Cand block_argmax_4(Cand c, Cand* sh) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(c.v, o, 64);
    const int i2 = __shfl_xor(c.i, o, 64);
    if (better(v2, i2, c.v, c.i)) { c.v = v2; c.i = i2; }
  }
  if (lane == 0) sh[wv] = c;
  __syncthreads();
  Cand r = sh[0];
  for (int w = 1; w < 4; ++w)
    if (better(sh[w].v, sh[w].i, r.v, r.i)) r = sh[w];
  return r;
}
template <int D>
__global__ __launch_bounds__(256) void lang_head_kernel(const float* __restrict__ x, long long ldx,
                                                        const float* __restrict__ g, const float* __restrict__ b,
                                                        const bf16* __restrict__ E, int lang_begin, int n_langs,
                                                        const unsigned char* __restrict__ allowed, float eps,
                                                        float* __restrict__ probs, int* __restrict__ top_id,
                                                        float* __restrict__ top_prob, int row0, int* __restrict__ err) {
  constexpr int NP = D / 128;                 // float2 pairs per lane (layernorm_kernel<NP>)
  constexpr int NC = D / 8;                   // 16-B chunks per embedding row
  constexpr int NS = (NC + 63) / 64;          // chunks per lane
  __shared__ __attribute__((aligned(16))) bf16 s_h[D];
  __shared__ float s_lg[LANG_MAX];
  __shared__ float sh[4];
  __shared__ Cand sh_c[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // 1. LayerNorm: every wave computes the row's statistics as layernorm_kernel's one wave does
  {
    const float2* xr = (const float2*)(x + (long long)row * ldx);
    float2 v[NP];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      v[i] = xr[lane + 64 * i];
      s += v[i].x + v[i].y;
    }
    const float mean = wave_sum(s) * (1.0f / D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const float a = v[i].x - mean, c = v[i].y - mean;
      q += a * a + c * c;
    }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / D) + eps);
    const float2* g2 = (const float2*)g;
    const float2* b2 = (const float2*)b;
    bf16x2* hr = (bf16x2*)s_h;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      if ((i & 3) != wv) continue;            // the waves hold the same values: each stores a quarter of the pairs
      const int c = lane + 64 * i;
      const float2 gg = g2[c], bb = b2[c];
      bf16x2 o;
      o[0] = f2bf((v[i].x - mean) * rstd * gg.x + bb.x);
      o[1] = f2bf((v[i].y - mean) * rstd * gg.y + bb.y);
      hr[c] = o;
    }
  }
  __syncthreads();
  // 2. language logits
  bf16x8 h[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int c = lane + 64 * s;
    h[s] = ((const bf16x8*)s_h)[c < NC ? c : 0];
  }
  const bf16x8* Er = (const bf16x8*)(E + (long long)lang_begin * D);
  for (int j0 = wv; j0 < n_langs; j0 += 4 * LANG_LB) {
    bf16x8 w[LANG_LB][NS];
#pragma unroll
    for (int k = 0; k < LANG_LB; ++k) {
      const int j = min(j0 + 4 * k, n_langs - 1);        // clamped: the load count is static, the extra sums are dropped
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int c = lane + 64 * s;
        w[k][s] = Er[(long long)j * NC + (c < NC ? c : 0)];
      }
    }
#pragma unroll
    for (int k = 0; k < LANG_LB; ++k) {
      float acc = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (lane + 64 * s < NC) {
#pragma unroll
          for (int t = 0; t < 8; ++t) acc = fmaf(bf2f(h[s][t]), bf2f(w[k][s][t]), acc);
        }
      }
      acc = wave_sum(acc);
      const int j = j0 + 4 * k;
      if (lane == 0 && j < n_langs) s_lg[j] = acc;
    }
  }
  __syncthreads();
  // 3. mask, 4. softmax, 5. argmax (n_langs <= LANG_MAX < 256: one language per thread)
  float lg = -INFINITY;
  if (tid < n_langs) {
    const float v = s_lg[tid];
    if ((!allowed || allowed[tid]) && isfinite(v)) lg = v;
  }
  Cand best = block_argmax_4(Cand{lg, tid < n_langs ? tid : 0x7fffffff}, sh_c);
  const float m = best.v;
  if (!(m > -INFINITY)) {                                  // no allowed language with a finite logit
    if (tid == 0) {
      wm_report_error(err, WM_ERR_NONFINITE, row0 + row, 0);
      top_id[row] = -1;
      top_prob[row] = 0.f;
    }
    if (tid < n_langs) probs[(long long)row * n_langs + tid] = 0.f;
    return;
  }
  float s = tid < n_langs ? expf(lg - m) : 0.f;
  s = wave_sum(s);
  if (lane == 0) sh[wv] = s;
  __syncthreads();
  s = sh[0] + sh[1] + sh[2] + sh[3];
  const float p = expf(lg - m) / s;                        // masked: expf(-inf) = 0, exactly 0 / s
  if (tid < n_langs) probs[(long long)row * n_langs + tid] = p;
  if (tid == best.i) {
    top_id[row] = tid;
    top_prob[row] = p;
  }
}

void launch_lang_head(const float* x, long long ldx, int rows, int d, const float* g, const float* b, const bf16* E,
                      int lang_begin, int n_langs, const unsigned char* allowed, float* probs, int* top_id,
                      float* top_prob, int row0, int* err, hipStream_t st) {
  if (rows <= 0) return;
  if (n_langs <= 0 || n_langs > LANG_MAX) throw std::runtime_error("lang_head: n_langs outside 1.." + std::to_string(LANG_MAX));
  if (ldx % 2 != 0) throw std::runtime_error("lang_head: odd row stride");
  const float eps = 1e-5f;
  const dim3 grid(rows), block(256);
#define LANG_HEAD(DD)                                                                                              \
  hipLaunchKernelGGL(lang_head_kernel<DD>, grid, block, 0, st, x, ldx, g, b, E, lang_begin, n_langs, allowed, eps, \
                     probs, top_id, top_prob, row0, err)
  switch (d) {
    case 384: LANG_HEAD(384); break;
    case 512: LANG_HEAD(512); break;
    case 768: LANG_HEAD(768); break;
    case 1024: LANG_HEAD(1024); break;
    case 1280: LANG_HEAD(1280); break;
    default: throw std::runtime_error("lang_head: unsupported width " + std::to_string(d));
  }
#undef LANG_HEAD
  WM_LAUNCH_CHECK("lang_head_kernel");
}

// wm_generate_multilingual: entry i = (ent[2i], ent[2i + 1]) puts the language token chosen for auto window ent[2i + 1]
// into table[ent[2i]].  A window whose head failed (top < 0; the call then fails at its end) keeps its placeholder.
__global__ __launch_bounds__(256) void lang_assign_kernel(int n, const int* __restrict__ ent, const int* __restrict__ top,
                                                          int lang_begin, int n_langs, int* __restrict__ table) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = top[ent[2 * i + 1]];
  if (t >= 0 && t < n_langs) table[ent[2 * i]] = lang_begin + t;
}

void launch_lang_assign(int n, const int* ent, const int* top, int lang_begin, int n_langs, int* table, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(lang_assign_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, ent, top, lang_begin, n_langs, table);
  WM_LAUNCH_CHECK("lang_assign_kernel");
}

// softmax(logits[r])[no_speech]
__global__ __launch_bounds__(SB) void no_speech_kernel(const float* __restrict__ logits, long long ldl, int V, int ns,
                                                        float* __restrict__ out, const int* __restrict__ out_idx) {
  __shared__ Cand sh_c[NW];
  __shared__ float sh_f[NW];
  const float* lg = logits + (long long)blockIdx.x * ldl;
  Cand m{-INFINITY, 0};
  for (int i = threadIdx.x; i < V; i += SB)
    if (lg[i] > m.v) { m.v = lg[i]; m.i = i; }
  m = block_argmax(m, sh_c);
  float s = 0.f;
  for (int i = threadIdx.x; i < V; i += SB) s += expf(lg[i] - m.v);
  s = block_sum(s, sh_f);
  if (threadIdx.x == 0) out[out_idx ? out_idx[blockIdx.x] : blockIdx.x] = expf(lg[ns] - m.v) / s;
}

void launch_no_speech(const float* logits, long long ldl, int V, int rows, int no_speech, float* out, hipStream_t st,
                      const int* out_idx) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(no_speech_kernel, dim3(rows), dim3(SB), 0, st, logits, ldl, V, no_speech, out, out_idx);
  WM_LAUNCH_CHECK("no_speech_kernel");
}
