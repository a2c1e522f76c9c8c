// Elementwise kernels: frame pre/post-processing, activations, resampling.
//
// Replaces (MI355X-natively) reference N3/N4 — CV-CUDA convertto + reformat
// (reference lib/pipeline.py:61-63) — and the wrapper's tensor post-process
// (reference lib/pipeline.py:72-74). All kernels vectorize to 8-16 B/lane
// (guide G13: scalar f16 ~2-2.5x slower) and grid-stride over capped grids
// (guide G11).

#include "common.h"
#include "yuv_math.h"

#define EW_BLOCK 256
#define EW_MAX_BLOCKS 2048

// ---------------------------------------------------------------------------
// u8 RGB -> f16 in [-1, 1]    (n = total element count, any; the last n % 8
// elements are written one by one by the first lanes of block 0, same launch)
// ---------------------------------------------------------------------------
__global__ void preprocess_u8_kernel(const uint8_t* __restrict__ in,
                                     f16* __restrict__ out, long n8, int tail) {
  const float inv = 1.0f / 127.5f;
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
    const long t = n8 * 8 + threadIdx.x;
    out[t] = (f16)((float)in[t] * inv - 1.0f);
  }
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += gridDim.x * blockDim.x) {
    // 8 u8 in, 8 f16 out per lane
    uint2 raw = reinterpret_cast<const uint2*>(in)[i];
    f16x8 o;
    const uint8_t* b = reinterpret_cast<const uint8_t*>(&raw);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)((float)b[j] * inv - 1.0f);
    reinterpret_cast<f16x8*>(out)[i] = o;
  }
}

extern "C" void airtc_preprocess_u8(const uint8_t* in, uint16_t* out, long n,
                                    hipStream_t s) {
  if (n <= 0) return;
  long n8 = n / 8;
  int blocks = (int)min((long)EW_MAX_BLOCKS, (n8 + EW_BLOCK - 1) / EW_BLOCK);
  if (blocks < 1) blocks = 1;  // n < 8: the tail lanes alone
  hipLaunchKernelGGL(preprocess_u8_kernel, dim3(blocks), dim3(EW_BLOCK), 0, s,
                     in, reinterpret_cast<f16*>(out), n8, (int)(n - n8 * 8));
}

// ---------------------------------------------------------------------------
// f16 in [-1,1] -> u8 with round+clamp (reference lib/pipeline.py:74);
// post_u8 is in common.h
// ---------------------------------------------------------------------------
// n any: the last n % 8 elements go one by one, as in preprocess_u8_kernel
__global__ void postprocess_u8_kernel(const f16* __restrict__ in,
                                      uint8_t* __restrict__ out, long n8,
                                      int tail) {
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
    const long t = n8 * 8 + threadIdx.x;
    out[t] = post_u8(in[t]);
  }
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += gridDim.x * blockDim.x) {
    f16x8 v = reinterpret_cast<const f16x8*>(in)[i];
    uint2 packed;
    uint8_t* b = reinterpret_cast<uint8_t*>(&packed);
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = post_u8(v[j]);
    reinterpret_cast<uint2*>(out)[i] = packed;
  }
}

extern "C" void airtc_postprocess_u8(const uint16_t* in, uint8_t* out, long n,
                                     hipStream_t s) {
  if (n <= 0) return;
  long n8 = n / 8;
  int blocks = (int)min((long)EW_MAX_BLOCKS, (n8 + EW_BLOCK - 1) / EW_BLOCK);
  if (blocks < 1) blocks = 1;  // n < 8: the tail lanes alone
  hipLaunchKernelGGL(postprocess_u8_kernel, dim3(blocks), dim3(EW_BLOCK), 0, s,
                     reinterpret_cast<const f16*>(in), out, n8,
                     (int)(n - n8 * 8));
}

// ---------------------------------------------------------------------------
// silu (f16, vec8)
// ---------------------------------------------------------------------------
__global__ void silu_kernel(const f16* __restrict__ in, f16* __restrict__ out,
                            long n8) {
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += gridDim.x * blockDim.x) {
    f16x8 v = reinterpret_cast<const f16x8*>(in)[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (f16)siluf((float)v[j]);
    reinterpret_cast<f16x8*>(out)[i] = v;
  }
}

extern "C" void airtc_silu_f16(const uint16_t* in, uint16_t* out, long n,
                               hipStream_t s) {
  long n8 = n / 8;
  int blocks = (int)min((long)EW_MAX_BLOCKS, (n8 + EW_BLOCK - 1) / EW_BLOCK);
  hipLaunchKernelGGL(silu_kernel, dim3(blocks), dim3(EW_BLOCK), 0, s,
                     reinterpret_cast<const f16*>(in),
                     reinterpret_cast<f16*>(out), n8);
}

// ---------------------------------------------------------------------------
// GEGLU: x (rows, 2*inner) -> a * gelu(b), out (rows, inner)
// ---------------------------------------------------------------------------
__global__ void geglu_kernel(const f16* __restrict__ in, f16* __restrict__ out,
                             long rows, long inner8) {
  long total = rows * inner8;
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    long r = i / inner8, c8 = i % inner8;
    const f16x8* row = reinterpret_cast<const f16x8*>(in + r * inner8 * 16);
    f16x8 a = row[c8];
    f16x8 b = row[c8 + inner8];
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)((float)a[j] * geluf((float)b[j]));
    reinterpret_cast<f16x8*>(out)[i] = o;
  }
}

extern "C" void airtc_geglu_f16(const uint16_t* in, uint16_t* out, long rows,
                                long inner, hipStream_t s) {
  long inner8 = inner / 8;
  long total = rows * inner8;
  int blocks = (int)min((long)EW_MAX_BLOCKS, (total + EW_BLOCK - 1) / EW_BLOCK);
  hipLaunchKernelGGL(geglu_kernel, dim3(blocks), dim3(EW_BLOCK), 0, s,
                     reinterpret_cast<const f16*>(in),
                     reinterpret_cast<f16*>(out), rows, inner8);
}

// ---------------------------------------------------------------------------
// fused add (+ optional activation): residual adds / TAESD add+relu
// ---------------------------------------------------------------------------
__global__ void add_act_kernel(const f16* __restrict__ a,
                               const f16* __restrict__ b, f16* __restrict__ out,
                               long n8, int act) {
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += gridDim.x * blockDim.x) {
    f16x8 va = reinterpret_cast<const f16x8*>(a)[i];
    f16x8 vb = reinterpret_cast<const f16x8*>(b)[i];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      va[j] = (f16)apply_act((float)va[j] + (float)vb[j], act);
    reinterpret_cast<f16x8*>(out)[i] = va;
  }
}

extern "C" void airtc_add_act_f16(const uint16_t* a, const uint16_t* b,
                                  uint16_t* out, long n, int act,
                                  hipStream_t s) {
  long n8 = n / 8;
  int blocks = (int)min((long)EW_MAX_BLOCKS, (n8 + EW_BLOCK - 1) / EW_BLOCK);
  hipLaunchKernelGGL(add_act_kernel, dim3(blocks), dim3(EW_BLOCK), 0, s,
                     reinterpret_cast<const f16*>(a),
                     reinterpret_cast<const f16*>(b),
                     reinterpret_cast<f16*>(out), n8, act);
}

// ---------------------------------------------------------------------------
// nearest-2x upsample, NHWC (C % 8 == 0)
// ---------------------------------------------------------------------------
__global__ void upsample2x_kernel(const f16* __restrict__ in,
                                  f16* __restrict__ out, int B, int H, int W,
                                  int C8) {
  long total = (long)B * 2 * H * 2 * W * C8;
  int W2 = 2 * W;
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    long c8 = i % C8;
    long rest = i / C8;
    int wo = rest % W2;
    rest /= W2;
    int ho = rest % (2 * H);
    long b = rest / (2 * H);
    long src = ((b * H + (ho >> 1)) * W + (wo >> 1)) * C8 + c8;
    reinterpret_cast<f16x8*>(out)[i] =
        reinterpret_cast<const f16x8*>(in)[src];
  }
}

extern "C" void airtc_upsample2x_f16(const uint16_t* in, uint16_t* out, int B,
                                     int H, int W, int C, hipStream_t s) {
  int C8 = C / 8;
  long total = (long)B * 2 * H * 2 * W * C8;
  int blocks = (int)min((long)EW_MAX_BLOCKS, (total + EW_BLOCK - 1) / EW_BLOCK);
  hipLaunchKernelGGL(upsample2x_kernel, dim3(blocks), dim3(EW_BLOCK), 0, s,
                     reinterpret_cast<const f16*>(in),
                     reinterpret_cast<f16*>(out), B, H, W, C8);
}

// ---------------------------------------------------------------------------
// Fused scheduler math (ROADMAP micro-fusion tier): the per-frame LCM
// scheduler steps were ~6 small aten broadcast kernels; each becomes ONE
// vectorized kernel with the per-batch-row coefficients read from f32
// arrays. per_b8 = elements-per-batch-row / 8.
//   add_noise:  out = a[b]*x0 + bt[b]*noise
//   blend:      out = c_out[b]*(x_t - bt[b]*eps)/a[b] + c_skip[b]*x_t
// ---------------------------------------------------------------------------
__global__ void sched_add_noise_kernel(const f16* __restrict__ x0,
                                       const f16* __restrict__ noise,
                                       const float* __restrict__ a,
                                       const float* __restrict__ bt,
                                       f16* __restrict__ out, long per_b8,
                                       long n8) {
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += gridDim.x * blockDim.x) {
    const long b = i / per_b8;
    const float av = a[b], bv = bt[b];
    f16x8 x = reinterpret_cast<const f16x8*>(x0)[i];
    f16x8 nz = reinterpret_cast<const f16x8*>(noise)[i];
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = (f16)(av * (float)x[j] + bv * (float)nz[j]);
    reinterpret_cast<f16x8*>(out)[i] = o;
  }
}

__global__ void sched_blend_kernel(const f16* __restrict__ xt,
                                   const f16* __restrict__ eps,
                                   const float* __restrict__ a,
                                   const float* __restrict__ bt,
                                   const float* __restrict__ c_out,
                                   const float* __restrict__ c_skip,
                                   f16* __restrict__ out, long per_b8,
                                   long n8) {
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += gridDim.x * blockDim.x) {
    const long b = i / per_b8;
    const float inv_a = 1.0f / a[b], bv = bt[b];
    const float co = c_out[b], cs = c_skip[b];
    f16x8 x = reinterpret_cast<const f16x8*>(xt)[i];
    f16x8 e = reinterpret_cast<const f16x8*>(eps)[i];
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xf = (float)x[j];
      const float x0 = (xf - bv * (float)e[j]) * inv_a;
      o[j] = (f16)(co * x0 + cs * xf);
    }
    reinterpret_cast<f16x8*>(out)[i] = o;
  }
}

extern "C" void airtc_sched_add_noise(const uint16_t* x0,
                                      const uint16_t* noise, const float* a,
                                      const float* bt, uint16_t* out,
                                      long per_b, long n, hipStream_t s) {
  const long n8 = n / 8;
  int blocks = (int)min((long)EW_MAX_BLOCKS, (n8 + EW_BLOCK - 1) / EW_BLOCK);
  hipLaunchKernelGGL(sched_add_noise_kernel, dim3(blocks), dim3(EW_BLOCK), 0,
                     s, reinterpret_cast<const f16*>(x0),
                     reinterpret_cast<const f16*>(noise), a, bt,
                     reinterpret_cast<f16*>(out), per_b / 8, n8);
}

extern "C" void airtc_sched_blend(const uint16_t* xt, const uint16_t* eps,
                                  const float* a, const float* bt,
                                  const float* c_out, const float* c_skip,
                                  uint16_t* out, long per_b, long n,
                                  hipStream_t s) {
  const long n8 = n / 8;
  int blocks = (int)min((long)EW_MAX_BLOCKS, (n8 + EW_BLOCK - 1) / EW_BLOCK);
  hipLaunchKernelGGL(sched_blend_kernel, dim3(blocks), dim3(EW_BLOCK), 0, s,
                     reinterpret_cast<const f16*>(xt),
                     reinterpret_cast<const f16*>(eps), a, bt, c_out, c_skip,
                     reinterpret_cast<f16*>(out), per_b / 8, n8);
}

// ---------------------------------------------------------------------------
// rcfg_apply: the residual-CFG step in ONE launch, coefficients per batch row
// from f32 device arrays (rewritten in place under a captured graph — one
// serving slot changes its guidance without touching the others). Replaces
// the ~6 aten launches of ResidualCFG.apply + _shift_stock. B = output rows.
//   SELF: out[r] = eps[r] + gm1[r]*(eps[r] - delta[r]*stock[r])
//         stock[r] <- eps[r] (r < fbs) | eps[r-fbs]          (the stage shift)
//   INIT: eps = [seed(fbs) | eps_c(B)]; as SELF on eps_c, rows r < fbs read
//         seed[r] where SELF reads stock[r]
//   FULL: eps = [eps_u(B) | eps_c(B)]; out[r] = eps_u[r] + g[r]*(eps_c[r]-eps_u[r])
//         (g arrives in the gm1 argument; no stock)
// Every arithmetic step rounds to f16, as the aten f16 chain does (f32 math,
// one rounding per op): with uniform coefficients the result is bit-identical
// to that chain, and the roundings keep the compiler from contracting across
// steps. Stock hazard: a thread reads stock[r][i] before it writes the same
// element and its other source (eps) is read-only, so the in-place shift
// needs no second buffer. T = f16x8 (per_b % 8 == 0) or f16 (any per_b);
// per_bv / nv count T-sized units per row / in the output.
// ---------------------------------------------------------------------------
enum RcfgMode { RCFG_SELF = 0, RCFG_INIT = 1, RCFG_FULL = 2 };

// f32 coefficient x f16 value: the product is rounded to f32 and THEN to
// f16, as aten's vectorized f16 kernels and its CPU kernels do. The empty
// asm keeps the multiply and the conversion apart: left alone the compiler
// may pick a mixed-precision multiply that rounds straight to f16, and the
// two disagree wherever the f32 rounding lands on an f16 tie (measured: the
// scalar path did, the f16x8 path did not). Sums and differences of two f16
// values need no such care, f32 holds them closely enough (24 >= 2*11 + 2)
// for the second rounding to be innocuous.
__device__ __forceinline__ f16 rcfg_scale(float c, f16 x) {
  float p = c * (float)x;
  asm volatile("" : "+v"(p));
  return (f16)p;
}

__device__ __forceinline__ f16 rcfg_self1(f16 e, f16 s, float gm1, float dl) {
  const f16 ds = rcfg_scale(dl, s);
  const f16 df = (f16)((float)e - (float)ds);
  const f16 sc = rcfg_scale(gm1, df);
  return (f16)((float)e + (float)sc);
}

__device__ __forceinline__ f16 rcfg_full1(f16 u, f16 c, float g) {
  const f16 df = (f16)((float)c - (float)u);
  const f16 sc = rcfg_scale(g, df);
  return (f16)((float)u + (float)sc);
}

__device__ __forceinline__ f16 rcfg_self(f16 e, f16 s, float gm1, float dl) {
  return rcfg_self1(e, s, gm1, dl);
}
__device__ __forceinline__ f16x8 rcfg_self(f16x8 e, f16x8 s, float gm1,
                                           float dl) {
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = rcfg_self1(e[j], s[j], gm1, dl);
  return o;
}
__device__ __forceinline__ f16 rcfg_full(f16 u, f16 c, float g) {
  return rcfg_full1(u, c, g);
}
__device__ __forceinline__ f16x8 rcfg_full(f16x8 u, f16x8 c, float g) {
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = rcfg_full1(u[j], c[j], g);
  return o;
}

template <int MODE, typename T>
__global__ void rcfg_apply_kernel(const T* __restrict__ eps, T* stock,
                                  const float* __restrict__ gm1,
                                  const float* __restrict__ delta,
                                  T* __restrict__ out, long B, long fbs,
                                  long per_bv, long nv) {
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < nv;
       i += gridDim.x * blockDim.x) {
    const long r = i / per_bv;
    if (MODE == RCFG_FULL) {
      out[i] = rcfg_full(eps[i], eps[B * per_bv + i], gm1[r]);
    } else {
      // conditional rows start after the seed rows in INIT
      const T* eps_c = MODE == RCFG_INIT ? eps + fbs * per_bv : eps;
      const T e = eps_c[i];
      const bool first = r < fbs;
      const T s = (MODE == RCFG_INIT && first) ? eps[i] : stock[i];
      out[i] = rcfg_self(e, s, gm1[r], delta[r]);
      stock[i] = first ? e : eps_c[i - fbs * per_bv];
    }
  }
}

template <typename T>
static void rcfg_apply_launch(int mode, const T* eps, T* stock,
                              const float* gm1, const float* delta, T* out,
                              long B, long fbs, long per_bv, hipStream_t s) {
  const long nv = B * per_bv;
  int blocks = (int)min((long)EW_MAX_BLOCKS, (nv + EW_BLOCK - 1) / EW_BLOCK);
  if (blocks < 1) return;
#define RCFG_LAUNCH(M)                                                       \
  hipLaunchKernelGGL((rcfg_apply_kernel<M, T>), dim3(blocks), dim3(EW_BLOCK), \
                     0, s, eps, stock, gm1, delta, out, B, fbs, per_bv, nv)
  if (mode == RCFG_SELF) RCFG_LAUNCH(RCFG_SELF);
  else if (mode == RCFG_INIT) RCFG_LAUNCH(RCFG_INIT);
  else RCFG_LAUNCH(RCFG_FULL);
#undef RCFG_LAUNCH
}

// vec != 0: per_b % 8 == 0 and every pointer 16-byte aligned (caller checks)
extern "C" void airtc_rcfg_apply(int mode, const uint16_t* eps,
                                 uint16_t* stock, const float* gm1,
                                 const float* delta, uint16_t* out, long B,
                                 long fbs, long per_b, int vec,
                                 hipStream_t s) {
  if (vec)
    rcfg_apply_launch(mode, reinterpret_cast<const f16x8*>(eps),
                      reinterpret_cast<f16x8*>(stock), gm1, delta,
                      reinterpret_cast<f16x8*>(out), B, fbs, per_b / 8, s);
  else
    rcfg_apply_launch(mode, reinterpret_cast<const f16*>(eps),
                      reinterpret_cast<f16*>(stock), gm1, delta,
                      reinterpret_cast<f16*>(out), B, fbs, per_b, s);
}

// ---------------------------------------------------------------------------
// fit_resize_u8: any-resolution ingest. One launch crops a source window
// (y0, x0, ch, cw) out of a u8 RGB NHWC frame, resizes it with the separable
// antialiased triangle filter (the filter of F.interpolate(mode="bilinear",
// antialias=True, align_corners=False)) into the destination window
// (oy, ox, oh, ow) of ONE (H, W, 3) u8 slot, and writes 0 everywhere else in
// that slot (the `contain` bars). Per axis, scale = n_in/n_out,
// sup = max(scale, 1), centre c = (o+0.5)*scale, taps
// [max(int(c-sup+0.5), 0), min(int(c+sup+0.5), n_in)), weight
// max(0, 1-|(j-c+0.5)/sup|) normalised to sum 1; taps clamp to the WINDOW.
//
// Shape: a workgroup owns a destination tile of FIT_TH rows x FIT_TW pixels
// and one lane owns one channel column of it (FIT_COLS = 3*FIT_TW lanes, so
// LDS reads/writes and the u8 stores are lane-consecutive). The source rows
// the tile needs are consumed in chunks of FIT_ROWS: horizontal pass
// global u8 -> f32 LDS (4 rows per step so 4 loads are in flight per tap),
// then the vertical pass accumulates that chunk's contribution out of LDS
// into FIT_TH f32 registers. Tap loops and the chunk loop are sized from
// the scale at run time, so LDS is fixed (24 KB) and NO downscale factor
// truncates taps. Source access is byte-wise: no pitch/alignment
// assumptions (Ws*3 need not be a multiple of 4).
//
// I420 = true is the egress form (fit_resize_u8_i420): the destination window
// is the whole (H, W) picture, H and W even, and dst is its I420 frame
// (H*W bytes of Y, then (H/2)*(W/2) of Cb, then of Cr, all tight). The tile is
// computed exactly as above; its rounded u8 values are staged in LDS (the
// `rows` array is free once the chunk loop is over) and leave the workgroup
// as planes: one lane per Y pixel, then one lane per chroma sample, both
// lane-consecutive along a row. FIT_TH and FIT_TW are even, so a 2x2 chroma
// block never straddles workgroups and no RGB picture is ever written.
// ---------------------------------------------------------------------------
#define FIT_TW 64
#define FIT_TH 8
#define FIT_COLS (FIT_TW * 3)
#define FIT_ROWS 32

// fit_taps (the tap window of an output pixel) is in common.h

__device__ __forceinline__ float fit_weight(float d, float inv_sup) {
  return fmaxf(0.0f, 1.0f - fabsf(d * inv_sup));
}

template <bool I420>
__global__ __launch_bounds__(FIT_COLS) void fit_resize_u8_kernel(
    const uint8_t* __restrict__ src, long spitch, uint8_t* __restrict__ dst,
    int H, int W, int y0, int x0, int ch, int cw, int oy, int ox, int oh,
    int ow) {
  __shared__ float rows[FIT_ROWS * FIT_COLS];
  const int tid = threadIdx.x;
  const int col = blockIdx.x * FIT_COLS + tid;  // dst channel column
  const int px = col / 3, chn = col - px * 3;
  const int ty0 = blockIdx.y * FIT_TH;
  const bool col_ok = col < W * 3;
  const bool in_x = col_ok && px >= ox && px < ox + ow;

  const double sx = (double)cw / ow, sy = (double)ch / oh;
  const double supx = fmax(sx, 1.0), supy = fmax(sy, 1.0);
  const float isupx = (float)(1.0 / supx), isupy = (float)(1.0 / supy);

  // horizontal taps of this lane's pixel: xs.., xn taps, fx = xs-c+0.5
  int xs = 0, xn = 0;
  float fx = 0.0f, inv_nx = 0.0f;
  if (in_x) {
    int xe;
    double c;
    fit_taps(px - ox, sx, supx, cw, xs, xe, c);
    xn = xe - xs;
    fx = (float)(xs - c + 0.5);
    float sum = 0.0f;
    for (int k = 0; k < xn; ++k) sum += fit_weight(fx + k, isupx);
    inv_nx = 1.0f / sum;
  }

  // vertical taps of the tile's rows (block-uniform); rows outside the
  // destination window keep zero taps and are written as 0
  int ys[FIT_TH], ye[FIT_TH];
  float dy[FIT_TH], inv_ny[FIT_TH], acc[FIT_TH];
  int ylo = 0, yhi = 0;
  bool any = false;
#pragma unroll
  for (int t = 0; t < FIT_TH; ++t) {
    const int o = ty0 + t - oy;
    ys[t] = ye[t] = 0;
    dy[t] = inv_ny[t] = acc[t] = 0.0f;
    if (o >= 0 && o < oh) {
      double c;
      fit_taps(o, sy, supy, ch, ys[t], ye[t], c);
      if (!any) ylo = ys[t];
      any = true;
      yhi = ye[t];
      // weight argument (j - c + 0.5) == (j - ylo) - dy
      dy[t] = (float)(c - 0.5 - ylo);
      float sum = 0.0f;
      for (int r = ys[t]; r < ye[t]; ++r)
        sum += fit_weight((float)(r - ylo) - dy[t], isupy);
      inv_ny[t] = 1.0f / sum;
    }
  }

  for (int r0 = ylo; r0 < yhi; r0 += FIT_ROWS) {
    const int nr = min(FIT_ROWS, yhi - r0);
    if (in_x) {
      const uint8_t* base =
          src + (long)(y0 + r0) * spitch + (long)(x0 + xs) * 3 + chn;
      for (int r = 0; r < nr; r += 4) {
        // rows past the chunk re-read its last row (in bounds, discarded)
        const uint8_t* p0 = base + (long)r * spitch;
        const uint8_t* p1 = base + (long)min(r + 1, nr - 1) * spitch;
        const uint8_t* p2 = base + (long)min(r + 2, nr - 1) * spitch;
        const uint8_t* p3 = base + (long)min(r + 3, nr - 1) * spitch;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        for (int k = 0; k < xn; ++k) {
          const float w = fit_weight(fx + k, isupx);
          a0 += w * (float)p0[k * 3];
          a1 += w * (float)p1[k * 3];
          a2 += w * (float)p2[k * 3];
          a3 += w * (float)p3[k * 3];
        }
        // FIT_ROWS % 4 == 0: r+3 stays inside the LDS tile
        rows[(r + 0) * FIT_COLS + tid] = a0 * inv_nx;
        rows[(r + 1) * FIT_COLS + tid] = a1 * inv_nx;
        rows[(r + 2) * FIT_COLS + tid] = a2 * inv_nx;
        rows[(r + 3) * FIT_COLS + tid] = a3 * inv_nx;
      }
    }
    __syncthreads();
    if (in_x) {
#pragma unroll
      for (int t = 0; t < FIT_TH; ++t) {
        const int a = max(ys[t], r0), b = min(ye[t], r0 + nr);
        for (int r = a; r < b; ++r)
          acc[t] += fit_weight((float)(r - ylo) - dy[t], isupy) *
                    rows[(r - r0) * FIT_COLS + tid];
      }
    }
    __syncthreads();
  }

  if (I420) {
    // the last __syncthreads() of the chunk loop released `rows`
    uint8_t* tile = reinterpret_cast<uint8_t*>(rows);
#pragma unroll
    for (int t = 0; t < FIT_TH; ++t) {
      // rows past H and columns past W have no taps: they stage 0 and are
      // never read back
      float v = in_x ? nearbyintf(acc[t] * inv_ny[t]) : 0.0f;
      v = fminf(255.0f, fmaxf(0.0f, v));
      tile[t * FIT_COLS + tid] = (uint8_t)v;
    }
    __syncthreads();
    const int tx0 = blockIdx.x * FIT_TW;
    const long plane = (long)H * W;
    // Y: one lane per pixel, FIT_TW consecutive lanes per tile row
    for (int i = tid; i < FIT_TH * FIT_TW; i += FIT_COLS) {
      const int ly = i / FIT_TW, lx = i - ly * FIT_TW;
      const int y = ty0 + ly, x = tx0 + lx;
      if (y < H && x < W) {
        const uint8_t* p = tile + ly * FIT_COLS + lx * 3;
        dst[(long)y * W + x] = luma_of(p[0], p[1], p[2]);
      }
    }
    // Cb, Cr: one lane per 2x2 block. H and W are even, so a block whose
    // top-left pixel is inside the picture is wholly inside it
    if (tid < (FIT_TH / 2) * (FIT_TW / 2)) {
      const int ly = tid / (FIT_TW / 2), lx = tid - ly * (FIT_TW / 2);
      const int y = ty0 + 2 * ly, x = tx0 + 2 * lx;
      if (y < H && x < W) {
        const uint8_t* p0 = tile + (2 * ly) * FIT_COLS + lx * 6;
        const uint8_t* p1 = p0 + FIT_COLS;
        const int R = (p0[0] + p0[3] + p1[0] + p1[3] + 2) >> 2;
        const int G = (p0[1] + p0[4] + p1[1] + p1[4] + 2) >> 2;
        const int B = (p0[2] + p0[5] + p1[2] + p1[5] + 2) >> 2;
        uint8_t cb, cr;
        chroma_of(R, G, B, cb, cr);
        // chroma planes are flat bytes: row pitch W/2 whatever H/2 is
        const long c = plane + (long)(y >> 1) * (W >> 1) + (x >> 1);
        dst[c] = cb;
        dst[c + plane / 4] = cr;
      }
    }
    return;
  }

  if (!col_ok) return;
#pragma unroll
  for (int t = 0; t < FIT_TH; ++t) {
    const int y = ty0 + t;
    if (y >= H) break;
    float v = in_x ? nearbyintf(acc[t] * inv_ny[t]) : 0.0f;
    v = fminf(255.0f, fmaxf(0.0f, v));
    dst[(long)y * W * 3 + col] = (uint8_t)v;
  }
}

extern "C" void airtc_fit_resize_u8(const uint8_t* src, int Ws, uint8_t* dst,
                                    int H, int W, int y0, int x0, int ch,
                                    int cw, int oy, int ox, int oh, int ow,
                                    hipStream_t s) {
  dim3 grid((W * 3 + FIT_COLS - 1) / FIT_COLS, (H + FIT_TH - 1) / FIT_TH);
  hipLaunchKernelGGL(fit_resize_u8_kernel<false>, grid, dim3(FIT_COLS), 0, s,
                     src, (long)Ws * 3, dst, H, W, y0, x0, ch, cw, oy, ox, oh,
                     ow);
}

// window (y0, x0, ch, cw) of src -> the whole (H, W) picture as I420 in dst
extern "C" void airtc_fit_resize_u8_i420(const uint8_t* src, int Ws,
                                         uint8_t* dst, int H, int W, int y0,
                                         int x0, int ch, int cw,
                                         hipStream_t s) {
  dim3 grid((W + FIT_TW - 1) / FIT_TW, (H + FIT_TH - 1) / FIT_TH);
  hipLaunchKernelGGL(fit_resize_u8_kernel<true>, grid, dim3(FIT_COLS), 0, s,
                     src, (long)Ws * 3, dst, H, W, y0, x0, ch, cw, 0, 0, H, W);
}
