// Fused normalisation kernels (NHWC).
//
// group_norm_silu: the UNet/ResNet GroupNorm(32)+SiLU pair fused into one
// kernel (reference runs these inside its TRT engine).
// One workgroup per (batch, group); two passes over the group's slice
// (sum/sumsq reduce, then normalise+affine+activation) with half2 loads.
//
// layer_norm: one wave per row (transformer blocks), f16x8 loads, two-pass
// f32 stats on deviations from the row's first element.

#include <stdlib.h>

#include "common.h"

// ---------------------------------------------------------------------------
// GroupNorm(+act) over NHWC: group g covers channels [g*Cg, (g+1)*Cg)
//
// TWO-PHASE, full-occupancy design: B*G is as small as 32 on SD shapes, so a
// one-block-per-group kernel leaves 224 of 256 CUs idle (measured 43us per
// call vs ~2us of traffic). Phase 1 spreads each group's stats over NCHUNK
// blocks (partial sum/sumsq slabs); phase 2 re-reads with the same grid,
// folding the tiny partial reduction into every block's prologue.
// ---------------------------------------------------------------------------
typedef __attribute__((__vector_size__(2 * sizeof(_Float16)))) _Float16 f16x2;

__device__ __forceinline__ void gn_chunk_range(long n2, int chunk, int nchunk,
                                               long* lo, long* hi) {
  const long per = (n2 + nchunk - 1) / nchunk;
  *lo = (long)chunk * per;
  *hi = min(n2, *lo + per);
}

__global__ void group_norm_stats_kernel(const f16* __restrict__ x,
                                        float* __restrict__ ws, int HW, int C,
                                        int G, int nchunk) {
  const int chunk = blockIdx.y;
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int Cg = C / G;
  const int Cg2 = Cg / 2;
  const long base = (long)b * HW * C + (long)g * Cg;
  long lo, hi;
  gn_chunk_range((long)HW * Cg2, chunk, nchunk, &lo, &hi);

  float sum = 0.f, sumsq = 0.f;
  for (long i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    long p = i / Cg2, c2 = i - p * Cg2;
    f16x2 v = *reinterpret_cast<const f16x2*>(&x[base + p * C + c2 * 2]);
    float a = (float)v[0], c = (float)v[1];
    sum += a + c;
    sumsq += a * a + c * c;
  }
  __shared__ float red[2][4];
  int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  sum = wave_reduce(sum, SumOp());
  sumsq = wave_reduce(sumsq, SumOp());
  if (lane == 0) { red[0][wid] = sum; red[1][wid] = sumsq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s0 = 0.f, s1 = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) { s0 += red[0][i]; s1 += red[1][i]; }
    float* w = &ws[((long)blockIdx.x * nchunk + chunk) * 2];
    w[0] = s0;
    w[1] = s1;
  }
}

// fold npart (sum, sumsq) partials, in index order, into the (mean, rstd) of
// a group of n elements (npart <= AIRTC_GN_MAX_PART: tiny, so every consumer
// block repeats it in its prologue instead of a separate launch)
__device__ __forceinline__ void gn_fold_partials(const float* w, int npart,
                                                 float n, float eps,
                                                 float* mean_out,
                                                 float* rstd_out) {
  float s0 = 0.f, s1 = 0.f;
  for (int i = 0; i < npart; ++i) { s0 += w[2 * i]; s1 += w[2 * i + 1]; }
  const float mean = s0 / n;
  *mean_out = mean;
  // one-pass variance: cancellation can take it below 0 on a near-constant
  // group, and rsqrtf of a negative argument is NaN
  *rstd_out = rsqrtf(fmaxf(s1 / n - mean * mean, 0.f) + eps);
}

// Q8: the apply pass writes OCP e4m3 CODES (q = clamp(act(gn(x)) * inv_sa,
// +-448)) instead of f16, so the fp8 conv stages raw bytes with zero encode
// VALU and half the activation HBM traffic (producer-side quantization — the
// conv's inline encode would otherwise re-encode every element once per 3x3
// tap). Encode uses the non-scaled v_cvt_pk_fp8_f32 (the scalef32 forms
// round up a ULP at arbitrary scales — see conv2d_fp8.hip header).
template <bool Q8>
__global__ void group_norm_apply_kernel(
    const f16* __restrict__ x, const float* __restrict__ ws,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    f16* __restrict__ out, uint8_t* __restrict__ outq, int HW, int C, int G,
    int nchunk, float eps, int act, float inv_sa) {
  const int chunk = blockIdx.y;
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int Cg = C / G;
  const int Cg2 = Cg / 2;
  const long base = (long)b * HW * C + (long)g * Cg;

  __shared__ float stats[2];
  if (threadIdx.x == 0)
    gn_fold_partials(&ws[(long)blockIdx.x * nchunk * 2], nchunk,
                     (float)HW * Cg, eps, &stats[0], &stats[1]);
  __syncthreads();
  const float mean = stats[0], rstd = stats[1];

  long lo, hi;
  gn_chunk_range((long)HW * Cg2, chunk, nchunk, &lo, &hi);
  for (long i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    long p = i / Cg2, c2 = i - p * Cg2;
    long idx = base + p * C + c2 * 2;
    f16x2 v = *reinterpret_cast<const f16x2*>(&x[idx]);
    int ch = g * Cg + (int)c2 * 2;
    float a[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float t = ((float)v[j] - mean) * rstd * gamma[ch + j] + beta[ch + j];
      a[j] = apply_act(t, act);
    }
    if (Q8) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        a[j] = fminf(fmaxf(a[j] * inv_sa, -448.0f), 448.0f);
      int p2 = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], 0, false);
      *reinterpret_cast<short*>(&outq[idx]) = (short)(p2 & 0xFFFF);
    } else {
      v[0] = (f16)a[0];
      v[1] = (f16)a[1];
      *reinterpret_cast<f16x2*>(&out[idx]) = v;
    }
  }
}

extern "C" int airtc_group_norm_nchunk(int B, int G) {
  int n = (int)(512 / max(1, B * G));
  if (n < 1) n = 1;
  if (n > 64) n = 64;
  return n;
}

// ---------------------------------------------------------------------------
// C % 8 == 0 fast path: 16 B accesses, no per-element integer division.
//
// A block is CT column lanes x PT pixel rows (PT = 256 / CT). Each lane owns
// 8 consecutive channels of the block's column tile and walks the block's
// pixel range, so the loop only advances a pointer. A 16 B vector may
// straddle group boundaries (Cg = 10, 30): statistics are therefore kept
// per CHANNEL in registers and folded to groups through LDS, and the apply
// pass reads per-channel (s, t) = (gamma*rstd, beta - mean*s) from an LDS
// table built in the prologue — one FMA plus the activation per element.
// The column tile is a whole number of groups (CT*8 == gpt*Cg), so every
// group's partial has exactly one writer: fixed-order, deterministic.
// Grid = (pixel chunks, column tiles, B).
// ---------------------------------------------------------------------------
struct GnPlan { int gpt, ct, pt; };

static bool gn_fast_plan(int C, int G, GnPlan* p) {
  if (G <= 0 || C % 8 != 0 || C % G != 0) return false;
  const int Cg = C / G;
  int gpt = 0;
  for (int d = 1; d <= G && d <= 64; ++d)
    if (G % d == 0 && (d * Cg) % 8 == 0 && d * Cg <= 512) gpt = d;
  if (!gpt) return false;
  p->gpt = gpt;
  p->ct = gpt * Cg / 8;
  p->pt = 256 / p->ct;
  return true;
}

__global__ __launch_bounds__(256) void group_norm_stats_v8_kernel(
    const f16* __restrict__ x, float* __restrict__ part, int HW, int C, int G,
    int ct, int per) {
  // pt * cw <= 2048 and cw <= 512 (gn_fast_plan)
  __shared__ float red[2][2048];
  __shared__ float col[2][512];
  const int cx = threadIdx.x % ct, py = threadIdx.x / ct;
  const int pt = 256 / ct;
  const int cw = ct * 8;
  const int b = blockIdx.z;
  const int p_lo = blockIdx.x * per;
  const int p_hi = min(HW, p_lo + per);
  if (py < pt) {
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
    const f16* xp = x + ((long)b * HW + p_lo + py) * C + blockIdx.y * cw + cx * 8;
    const long step = (long)pt * C;
#pragma unroll 2
    for (int p = p_lo + py; p < p_hi; p += pt, xp += step) {
      const f16x8 v = *reinterpret_cast<const f16x8*>(xp);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)v[j];
        s[j] += f;
        q[j] += f * f;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[0][py * cw + cx * 8 + j] = s[j];
      red[1][py * cw + cx * 8 + j] = q[j];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cw; c += 256) {
    float a0 = 0.f, a1 = 0.f;
    for (int r = 0; r < pt; ++r) {
      a0 += red[0][r * cw + c];
      a1 += red[1][r * cw + c];
    }
    col[0][c] = a0;
    col[1][c] = a1;
  }
  __syncthreads();
  const int Cg = C / G;
  const int gpt = cw / Cg;
  if ((int)threadIdx.x < gpt) {
    float a0 = 0.f, a1 = 0.f;
    for (int i = 0; i < Cg; ++i) {
      a0 += col[0][threadIdx.x * Cg + i];
      a1 += col[1][threadIdx.x * Cg + i];
    }
    const int g = blockIdx.y * gpt + threadIdx.x;
    float* w = part + (((long)b * G + g) * gridDim.x + blockIdx.x) * 2;
    w[0] = a0;
    w[1] = a1;
  }
}

// Q8: write e4m3 codes (see group_norm_apply_kernel) instead of f16
template <bool Q8>
__global__ __launch_bounds__(256) void group_norm_apply_v8_kernel(
    const f16* __restrict__ x, const float* __restrict__ part,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    f16* __restrict__ out, uint8_t* __restrict__ outq, int HW, int C, int G,
    int npart, float eps, int act, float inv_sa, int ct, int per) {
  __shared__ float gst[2][64];
  __shared__ float tab[2][512];
  const int cx = threadIdx.x % ct, py = threadIdx.x / ct;
  const int pt = 256 / ct;
  const int cw = ct * 8;
  const int b = blockIdx.z;
  const int ch0 = blockIdx.y * cw;
  const int Cg = C / G;
  const int gpt = cw / Cg;
  // fold the tiny cross-chunk reduction into every block (npart <= 64)
  if ((int)threadIdx.x < gpt) {
    const int g = blockIdx.y * gpt + threadIdx.x;
    gn_fold_partials(&part[((long)b * G + g) * npart * 2], npart,
                     (float)HW * Cg, eps, &gst[0][threadIdx.x],
                     &gst[1][threadIdx.x]);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cw; c += 256) {
    const int gi = c / Cg;
    const float sc = gamma[ch0 + c] * gst[1][gi];
    tab[0][c] = sc;
    tab[1][c] = beta[ch0 + c] - gst[0][gi] * sc;
  }
  __syncthreads();
  if (py >= pt) return;
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = tab[0][cx * 8 + j];
    sh[j] = tab[1][cx * 8 + j];
  }
  const int p_lo = blockIdx.x * per;
  const int p_hi = min(HW, p_lo + per);
  long idx = ((long)b * HW + p_lo + py) * C + ch0 + cx * 8;
  const long step = (long)pt * C;
#pragma unroll 2
  for (int p = p_lo + py; p < p_hi; p += pt, idx += step) {
    f16x8 v = *reinterpret_cast<const f16x8*>(&x[idx]);
    if (Q8) {
      float a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = (float)v[j] * sc[j] + sh[j];
        a[j] = fminf(fmaxf(apply_act(t, act) * inv_sa, -448.0f), 448.0f);
      }
      int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], 0, false);
      w0 = __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], w0, true);
      int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(a[4], a[5], 0, false);
      w1 = __builtin_amdgcn_cvt_pk_fp8_f32(a[6], a[7], w1, true);
      uint2 q;
      q.x = (uint32_t)w0;
      q.y = (uint32_t)w1;
      *reinterpret_cast<uint2*>(&outq[idx]) = q;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = (f16)apply_act((float)v[j] * sc[j] + sh[j], act);
      *reinterpret_cast<f16x8*>(&out[idx]) = v;
    }
  }
}

// stats launch of the fast path; returns the partial count it wrote
static int gn_launch_stats_v8(const GnPlan& pl, const f16* x, float* part,
                              int B, int HW, int C, int G, hipStream_t s) {
  const int n0 = min(64, ceil_div(HW, pl.pt));
  const int per = ceil_div(HW, n0);
  const int npart = ceil_div(HW, per);  // <= 64, no empty chunk
  hipLaunchKernelGGL(group_norm_stats_v8_kernel, dim3(npart, G / pl.gpt, B),
                     dim3(256), 0, s, x, part, HW, C, G, pl.ct, per);
  return npart;
}

static void gn_launch_apply_v8(const GnPlan& pl, const f16* x,
                               const float* part, int npart,
                               const float* gamma, const float* beta, f16* out,
                               uint8_t* outq, int B, int HW, int C, int G,
                               float eps, int act, float inv_sa,
                               hipStream_t s) {
  // ~512 blocks, at least one pixel per thread row
  const int tiles = G / pl.gpt;
  int nch = ceil_div(512, tiles * B);
  nch = max(1, min(nch, ceil_div(HW, pl.pt)));
  const int per = ceil_div(HW, nch);
  dim3 grid(ceil_div(HW, per), tiles, B);
  if (outq)
    hipLaunchKernelGGL(group_norm_apply_v8_kernel<true>, grid, dim3(256), 0, s,
                       x, part, gamma, beta, out, outq, HW, C, G, npart, eps,
                       act, inv_sa, pl.ct, per);
  else
    hipLaunchKernelGGL(group_norm_apply_v8_kernel<false>, grid, dim3(256), 0,
                       s, x, part, gamma, beta, out, outq, HW, C, G, npart,
                       eps, act, inv_sa, pl.ct, per);
}

static bool gn_fast_ok(const void* x, const void* out, int B, int C, int G,
                       GnPlan* pl) {
  // Opt-in (AIRTC_GN_FAST=1): measured SLOWER end-to-end on MI355X at SD
  // shapes (144.5/144.6 fps with it vs 145.7/146.8 without, same session;
  // 64x64x320 stats+apply 14.7 us vs 12.1 us): at B=1 the <= 64 pixel chunks per
  // column tile leave the stats pass on ~64 blocks of serial loads, where
  // the f16x2 kernels spread 512. Read per call so one process can run both.
  const char* e = getenv("AIRTC_GN_FAST");
  if (!(e && atoi(e) == 1) || B > 65535) return false;
  if ((((uintptr_t)x | (uintptr_t)out) & 15) != 0) return false;
  return gn_fast_plan(C, G, pl);
}

// per-(b, channel) affine pairs for the fused GN->conv input transform
// (conv2d.hip load_a): s = gamma_c * rstd_g, t = beta_c - mean_g * s.
// Replaces the full-tensor apply pass when the ONLY consumer is a conv.
__global__ void group_norm_coeffs_kernel(const float* __restrict__ ws,
                                         const float* __restrict__ gamma,
                                         const float* __restrict__ beta,
                                         float* __restrict__ coeffs, int HW,
                                         int C, int G, int nchunk,
                                         float eps) {
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int Cg = C / G;
  __shared__ float stats[2];
  if (threadIdx.x == 0)
    gn_fold_partials(&ws[(long)blockIdx.x * nchunk * 2], nchunk,
                     (float)HW * Cg, eps, &stats[0], &stats[1]);
  __syncthreads();
  const float mean = stats[0], rstd = stats[1];
  for (int c = threadIdx.x; c < Cg; c += blockDim.x) {
    const int ch = g * Cg + c;
    const float sc = gamma[ch] * rstd;
    float* o = &coeffs[((long)b * C + ch) * 2];
    o[0] = sc;
    o[1] = beta[ch] - mean * sc;
  }
}

extern "C" void airtc_group_norm_coeffs(const uint16_t* x, const float* gamma,
                                        const float* beta, float* coeffs,
                                        float* ws, int B, int HW, int C,
                                        int G, float eps, hipStream_t s) {
  const int nchunk = airtc_group_norm_nchunk(B, G);
  dim3 grid(B * G, nchunk);
  hipLaunchKernelGGL(group_norm_stats_kernel, grid, dim3(256), 0, s,
                     reinterpret_cast<const f16*>(x), ws, HW, C, G, nchunk);
  hipLaunchKernelGGL(group_norm_coeffs_kernel, dim3(B * G), dim3(256), 0, s,
                     ws, gamma, beta, coeffs, HW, C, G, nchunk, eps);
}

// GroupNorm + act, the one launcher. part == nullptr: run the statistics pass
// into ws first; otherwise apply on partial statistics somebody else produced
// (the split-K finalize, conv2d.hip): part is [B*G][npart][2], npart <= 64.
// Exactly one of out / out_q8 is non-null (f16 result, or e4m3 codes at
// a_scale).
extern "C" void airtc_group_norm(const uint16_t* x, const float* part,
                                 int npart, const float* gamma,
                                 const float* beta, uint16_t* out,
                                 uint8_t* out_q8, float* ws, int B, int HW,
                                 int C, int G, float eps, int act,
                                 float a_scale, hipStream_t s) {
  const f16* xp = reinterpret_cast<const f16*>(x);
  f16* op = reinterpret_cast<f16*>(out);
  const float inv_sa = out_q8 ? 1.0f / a_scale : 0.f;
  GnPlan pl;
  const bool fast = gn_fast_ok(
      x, out_q8 ? (const void*)out_q8 : (const void*)out, B, C, G, &pl);
  if (!part) {
    if (fast) {
      npart = gn_launch_stats_v8(pl, xp, ws, B, HW, C, G, s);
    } else {
      npart = airtc_group_norm_nchunk(B, G);
      hipLaunchKernelGGL(group_norm_stats_kernel, dim3(B * G, npart),
                         dim3(256), 0, s, xp, ws, HW, C, G, npart);
    }
    part = ws;
  }
  if (fast) {
    gn_launch_apply_v8(pl, xp, part, npart, gamma, beta, op, out_q8, B, HW, C,
                       G, eps, act, inv_sa, s);
    return;
  }
  // the f16x2 kernels chunk their own work by the partial count
  dim3 grid(B * G, npart);
  if (out_q8)
    hipLaunchKernelGGL(group_norm_apply_kernel<true>, grid, dim3(256), 0, s,
                       xp, part, gamma, beta, op, out_q8, HW, C, G, npart, eps,
                       act, inv_sa);
  else
    hipLaunchKernelGGL(group_norm_apply_kernel<false>, grid, dim3(256), 0, s,
                       xp, part, gamma, beta, op, out_q8, HW, C, G, npart, eps,
                       act, inv_sa);
}

// ---------------------------------------------------------------------------
// LayerNorm: rows x C, one wave per row (C % 8 == 0)
// ---------------------------------------------------------------------------
// NV > 0: the row fits NV f16x8 per lane (C8 <= NV * 64) and is read ONCE
// into registers; all three sweeps below run on them. NV == 0: any C8, the
// row is re-read from cache for each sweep.
template <int NV>
__global__ void layer_norm_kernel(const f16* __restrict__ x,
                                  const float* __restrict__ gamma,
                                  const float* __restrict__ beta,
                                  f16* __restrict__ out, long rows, int C8,
                                  float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const f16x8* xr = reinterpret_cast<const f16x8*>(x) + row * C8;
  constexpr int NR = NV > 0 ? NV : 1;
  f16x8 reg[NR];
  if (NV > 0) {
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int i = lane + k * WAVE;
      if (i < C8) reg[k] = xr[i];
    }
  }
  // body(i, v) over this lane's vectors of the row
  auto sweep = [&](auto body) {
    if constexpr (NV > 0) {
#pragma unroll
      for (int k = 0; k < NR; ++k) {
        const int i = lane + k * WAVE;
        if (i < C8) body(i, reg[k]);
      }
    } else {
      for (int i = lane; i < C8; i += WAVE) body(i, xr[i]);
    }
  };

  // Statistics on deviations from the row's first element: a difference of
  // two f16 values of similar magnitude is exact in f32 (otherwise it is one
  // f32 rounding), so a row far from zero (mean 64, std 0.25) keeps every
  // variance bit that sumsq/n - mean^2 cancels away.
  // Mean of the deviations first, then the centred sum of squares in a
  // second sweep.
  const float pivot = (float)x[row * C8 * 8];
  float sum = 0.f;
  sweep([&](int, const f16x8 v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += (float)v[j] - pivot;
  });
  sum = wave_reduce(sum, SumOp());
  const float n = (float)C8 * 8.0f;
  const float dmean = sum / n;
  float sumsq = 0.f;
  sweep([&](int, const f16x8 v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float c = ((float)v[j] - pivot) - dmean;
      sumsq += c * c;
    }
  });
  sumsq = wave_reduce(sumsq, SumOp());
  const float rstd = rsqrtf(fmaxf(sumsq / n, 0.f) + eps);

  f16x8* orow = reinterpret_cast<f16x8*>(out) + row * C8;
  sweep([&](int i, const f16x8 v) {
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = (f16)((((float)v[j] - pivot) - dmean) * rstd * gamma[i * 8 + j] +
                   beta[i * 8 + j]);
    orow[i] = o;
  });
}

extern "C" void airtc_layer_norm(const uint16_t* x, const float* gamma,
                                 const float* beta, uint16_t* out, long rows,
                                 int C, float eps, hipStream_t s) {
  int waves_per_block = 4;
  long blocks = (rows + waves_per_block - 1) / waves_per_block;
  const int C8 = C / 8;
#define LN_LAUNCH(NV)                                                      \
  hipLaunchKernelGGL(layer_norm_kernel<NV>, dim3((uint32_t)blocks),        \
                     dim3(waves_per_block * WAVE), 0, s,                   \
                     reinterpret_cast<const f16*>(x), gamma, beta,         \
                     reinterpret_cast<f16*>(out), rows, C8, eps)
  // C <= 2048: the row stays in registers (1..4 vectors per lane)
  if (C8 <= 1 * WAVE) LN_LAUNCH(1);
  else if (C8 <= 2 * WAVE) LN_LAUNCH(2);
  else if (C8 <= 3 * WAVE) LN_LAUNCH(3);
  else if (C8 <= 4 * WAVE) LN_LAUNCH(4);
  else LN_LAUNCH(0);
#undef LN_LAUNCH
}
