// Decoder attention: the host launchers of attn_dec.hip and attn_xenc.hip and the two deferred-rescale thresholds,
// declared once for the kernels, engine.cpp and the tools (tools/attn_check, tools/xattn_bench).
#pragma once

// Deferred rescale of the online softmax (log2 units): the running maximum m_run of a row is raised, and l / o are
// rescaled, only when a tile's maximum exceeds it by more than the threshold, so max_t s_t - THR <= m_run <= max_t s_t
// and P = 2^(s - m_run) stays below 2^THR before its bf16 rounding.
constexpr float XATTN_RESCALE_THR = 8.0f;      // xattn_kernel (attn_xenc.hip)
constexpr float CROSS_TF_RESCALE_THR = 8.0f;   // cross_tf_kernel (attn_dec.hip)

#ifndef ATTN_H_CONSTANTS_ONLY   // (a host-only program takes the constants alone: no HIP headers)
#include "common.h"

// ---- attn_dec.hip
// (q, ldq, k cache, v cache, lin, row_hyp, row_pos, done, out, ldo, rows, H, n_ctx, stat, stream, ev0, ev1, plan_rows, group)
void launch_self_attn(const bf16* q, long long ldq, const bf16* kc, const bf16* vc, const int* lin, const int* row_hyp,
                      const int* row_pos, const int* done, bf16* out, long long ldo, int rows, int H, int n_ctx,
                      unsigned long long* stat, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, int plan_rows, int group);
void launch_cross_attn(const bf16* q, long long ldq, const bf16* kbase, const bf16* vbase, int T, const int* hyp_slot,
                       const int* row_hyp, const int* done, bf16* out, long long ldo, int rows, int H, int group,
                       float* part_m, float* part_l, float* part_o, float* probs, const int* head_map, int n_align,
                       int plan_rows, int cap, const CrossFuse& fz, unsigned long long* stat, hipStream_t st,
                       hipEvent_t ev0, hipEvent_t ev1);
// The same operation on fp8 panels (common.h CrossKv8): same routing and split rules, the kernels' F8 instantiations,
// which convert a code to its exact bf16 value on load.  A slot table is required.
void launch_cross_attn_fp8(const bf16* q, long long ldq, const CrossKv8& kv, int T, const int* hyp_slot,
                           const int* row_hyp, const int* done, bf16* out, long long ldo, int rows, int H, int group,
                           float* part_m, float* part_l, float* part_o, float* probs, const int* head_map, int n_align,
                           int plan_rows, int cap, const CrossFuse& fz, unsigned long long* stat, hipStream_t st,
                           hipEvent_t ev0, hipEvent_t ev1);
// Quantiser of those panels: rows of 64 bf16 -> 64 codes + 1 exponent byte (deq == nullptr), or the dequantised bf16
// rows (deq != nullptr: the reference form).  Source row r goes to destination row
// (r / src_per) * dst_stride + dst_off + r % src_per.
void launch_kv8_quant(const bf16* src, long long n_rows, long long src_per, long long dst_stride, long long dst_off,
                      unsigned char* codes, unsigned char* exps, bf16* deq, hipStream_t st);

// ---- attn_xenc.hip: factored cross-attention over the encoder output
void launch_xpack(const bf16* ckv_w, bf16* wkt, bf16* wvb, int L, int H, int d, hipStream_t st);
void launch_xq(const bf16* q, long long ldq, const CrossFuse& fz, const bf16* wkt, bf16* qp, int rows, int H, int d,
               hipStream_t st);
int xattn_splits(int plan_rows, int group, int H, int T, int d);
void launch_xquant8(const bf16* enc, long long rows, int d, unsigned char* out, float* scale, hipStream_t st);
long long xblock_slot_elems(int T, int d);
void launch_xblock(const bf16* src, int B, int T, int d, bf16* dst, bool to_blocked, hipStream_t st);
void xattn_geometry(int d, int& qw, int& nw);
void launch_xattn(const bf16* qp, const void* enc, const float* escale, const int* hyp_slot, const int* row_hyp,
                  const int* done, int rows, long long slab_rows, int group, int H, int T, int d, int splits, int rev,
                  int keep, bf16* part_u, float* part_ml, float* probs, const int* head_map, int n_align,
                  unsigned long long* stat, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
void launch_xcomb_vo(const bf16* part_u, const float* part_ml, int splits, long long slab_rows, const bf16* wvb,
                     const float* bv, const int* row_hyp, const int* done, bf16* out, long long ldo, int rows, int H, int d,
                     int T, float* probs, const int* head_map, int n_align, hipStream_t st);
void xattn_set_ablation(int abl);
#endif
