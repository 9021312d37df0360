// Sample-rate conversion to 16 kHz on the device (wm_resample): interleaved s16 / f32 frames at any supported rate
// -> f32 mono, the polyphase FIR of scipy.signal.resample_poly's default filter (definition: include/whisper_mi355.h,
// vlog_amd/audio.py).
//
//   y[j] = sum_t mono[i_hi - t] * h[q + t up],  a = j down + half, i_hi = a / up, q = a mod up, t = 0 .. (2 half - q) / up
//
// A workgroup of 256 threads computes `tile` consecutive outputs.  It stages in LDS (a) the taps in polyphase order
// (not when up == 1: one phase, every lane reads the same tap, which then comes through the scalar unit),
// pp[q * T + t] = h[q + t up] (T >= ceil(N / up), odd; built once per ratio on the host, engine.cpp), and (b) the downmixed
// source frames the tile reads, [lo, hi] = [ceil((j0 down - half) / up), floor((j1 down + half) / up)] for the tile's
// first and last output: at most ((tile - 1) down + 2 half) / up + 2 frames.  Frames outside the file, and frames
// outside the span the caller holds (the host has checked that no output needs one of those), are staged as zero.
// Each output is then one thread's f32 fma chain over t ascending from zero: its value depends on the file and j
// alone, bit for bit, whatever the tile, the call's output range or its source span.
#include <stdexcept>
#include <string>

#include "common.h"

#define RS_THREADS 256

template <bool S16>
__device__ __forceinline__ float rs_frame(const void* __restrict__ src, long long f, int ch, int channel, float scale) {
  if (S16) {
    const short* p = (const short*)src + f * ch;
    if (channel >= 0) return (float)p[channel] * scale;
    int s = 0;                                       // exact: at most 8 channels of 16 bits
    if (ch == 2 && ((reinterpret_cast<uintptr_t>(p) & 3) == 0)) {
      const int v = *(const int*)p;
      s = (int)(short)(v & 0xffff) + (v >> 16);
    } else {
      for (int c = 0; c < ch; ++c) s += p[c];
    }
    return (float)s * scale;
  } else {
    const float* p = (const float*)src + f * ch;
    if (channel >= 0) return p[channel];
    float s = p[0];
    for (int c = 1; c < ch; ++c) s += p[c];           // channel order
    return s * scale;
  }
}

// d_src holds frames [src0, src0 + n_src); n_total < 0: the end of the file is not known (no frame at or past the
// span's end is needed).  span_cap: the LDS frames the launch reserved (host: rs_span_cap).
template <bool S16, bool UP1>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const void* __restrict__ src, int ch, int channel, float scale,
                                                              long long src0, long long n_src, long long n_total,
                                                              const float* __restrict__ pp, int up, int down, int half,
                                                              int T, long long out0, long long n_out, int tile,
                                                              int span_cap, float* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  float* s_pp = rs_lds;                               // [up * T] (UP1: not staged, see below)
  float* s_x = UP1 ? rs_lds : rs_lds + (size_t)up * T;   // [span_cap]
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * tile;  // first output of the tile, relative to out0
  if (r0 >= n_out) return;
  const int nt = (int)((n_out - r0 < tile) ? (n_out - r0) : tile);
  const long long j0 = out0 + r0;
  const long long num = j0 * down - half;
  const long long lo = num >= 0 ? (num + up - 1) / up : -((-num) / up);
  const long long a0 = j0 * down + half;              // >= 0
  const long long hi = (a0 + (long long)(nt - 1) * down) / up;
  long long ns = hi - lo + 1;
  if (ns > span_cap) ns = span_cap;                   // never: span_cap is the bound of hi - lo + 1 (guards the LDS)
  const long long f_end = n_total >= 0 ? n_total : src0 + n_src;
  if (lo >= 0 && lo >= src0 && lo + ns <= f_end && lo + ns <= src0 + n_src) {
    // the whole span is in the file and in the caller's buffer (every tile but those at the ends): no per-frame
    // test, so the loads of an unrolled group are in flight together
#pragma unroll 8
    for (int i = tid; i < (int)ns; i += RS_THREADS) s_x[i] = rs_frame<S16>(src, lo + i - src0, ch, channel, scale);
  } else {
    for (int i = tid; i < (int)ns; i += RS_THREADS) {
      const long long f = lo + i;
      float v = 0.f;
      if (f >= 0 && f < f_end && f >= src0 && f < src0 + n_src) v = rs_frame<S16>(src, f - src0, ch, channel, scale);
      s_x[i] = v;
    }
  }
  if (!UP1) {
    const int npp = up * T, npp4 = npp >> 2;          // pp is a device allocation of its own: 16-byte aligned
#pragma unroll 4
    for (int i = tid; i < npp4; i += RS_THREADS) ((f32x4*)s_pp)[i] = ((const f32x4*)pp)[i];
    for (int i = (npp4 << 2) + tid; i < npp; i += RS_THREADS) s_pp[i] = pp[i];
  }
  __syncthreads();
  const long long i0 = a0 / up;                       // i_hi of the tile's first output
  const int q0 = (int)(a0 - i0 * up);
  const int xb = (int)(i0 - lo);                      // its index in s_x
  for (int r = tid; r < nt; r += RS_THREADS) {
    float acc = 0.f;
    if (UP1) {
      // up == 1: one phase, so tap t is the same word for every lane: read from memory through the scalar unit
      // instead of an LDS broadcast (the fma chain is the same: same taps, same order)
      const float* __restrict__ xp = s_x + xb + r * down;
      const int n_t = 2 * half + 1;
      for (int t = 0; t < n_t; ++t) acc = fmaf(xp[-t], pp[t], acc);
    } else {
      const unsigned d = (unsigned)r * (unsigned)down + (unsigned)q0;    // < 2048 * 819 + 819
      const unsigned di = d / (unsigned)up;
      const int q = (int)(d - di * (unsigned)up);
      const int n_t = (2 * half - q) / up + 1;
      const float* __restrict__ hp = s_pp + q * T;
      const float* __restrict__ xp = s_x + xb + (int)di;
      for (int t = 0; t < n_t; ++t) acc = fmaf(xp[-t], hp[t], acc);
    }
    dst[r0 + r] = acc;
  }
}

// Outputs per workgroup for a ratio: as many as keep the staged span within RS_SPAN_MAX frames, at most 2048 (a
// multiple of the workgroup from 256 up; below that whatever fits, one at the least, which the widest ratio of the
// supported range, down = 819 with up = 1, still fits: 16380 + 2 frames).
#define RS_SPAN_MAX 17408
int rs_tile(int up, int down, int half) {
  const long long room = (long long)RS_SPAN_MAX - 3 - (2LL * half) / up;
  long long t = room * up / down + 1;                 // ((t - 1) down + 2 half) / up + 2 <= RS_SPAN_MAX
  if (t > 2048) t = 2048;
  if (t >= RS_THREADS) t -= t % RS_THREADS;
  return t < 1 ? 1 : (int)t;
}
int rs_span_cap(int up, int down, int half, int tile) {
  return (int)(((long long)(tile - 1) * down + 2LL * half) / up + 2);
}

void launch_resample(const void* src, int fmt, int ch, int channel, long long src0, long long n_src, long long n_total,
                     const float* pp, int up, int down, int half, int T, long long out0, long long n_out, float* dst,
                     hipStream_t st) {
  if (n_out <= 0) return;
  const int tile = rs_tile(up, down, half);
  const int cap = rs_span_cap(up, down, half, tile);
  const bool up1 = up == 1;                           // the taps are then read through the scalar unit, not staged
  const size_t lds = ((up1 ? 0 : (size_t)up * T) + cap) * sizeof(float);
  if (lds > 160 * 1024) throw std::runtime_error("resample_kernel: " + std::to_string(lds) + " bytes of LDS");
  const long long blocks = (n_out + tile - 1) / tile;
  if (blocks > 0x7fffffffLL) throw std::runtime_error("resample_kernel: too many outputs in one call");
  float scale;
  if (fmt == 0) scale = channel >= 0 ? 1.0f / 32768.0f : 1.0f / (32768.0f * (float)ch);
  else scale = channel >= 0 ? 1.0f : 1.0f / (float)ch;
  auto kern = fmt == 0 ? (up1 ? resample_kernel<true, true> : resample_kernel<true, false>)
                       : (up1 ? resample_kernel<false, true> : resample_kernel<false, false>);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) throw std::runtime_error(std::string("resample_kernel LDS attribute: ") + hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(RS_THREADS), lds, st, src, ch, channel, scale, src0, n_src,
                     n_total, pp, up, down, half, T, out0, n_out, tile, cap, dst);
  WM_LAUNCH_CHECK("resample_kernel");
}
