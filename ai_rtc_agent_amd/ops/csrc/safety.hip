// CLIP safety checker, the kernels at both ends of the ViT tower
// (models/safety_clip.py) and its activation:
//   clip_patches   decoder image -> the patch-embedding GEMM's A operand
//   quick_gelu     x * sigmoid(1.702 x)
//   safety_head    class token -> LayerNorm -> projection -> cosines ->
//                  decision, per frame, on the device
//   blank_flagged  flagged frames -> black, in place
// The definitions (preprocessing, decision law) are stated once, in
// ops/interface.py; the torch forms there are what these kernels compute.

#include "common.h"

#define EW_BLOCK 256
#define EW_MAX_BLOCKS 2048

// ---------------------------------------------------------------------------
// clip_patches: what CLIPImageProcessor does to the frame the viewer would
// get, in one launch. Per input pixel post_u8 (the u8 level postprocess_u8
// writes); separable antialiased bicubic resize (Keys a = -0.5, support
// 2*max(scale, 1), centres (o+0.5)*scale, taps clamped to the image and
// renormalised) to (nh, nw); round-half-even and clamp to u8; the size x size
// window at (top, left); (v/255 - mean)/std through a 3x256 f16 table built
// by the host; written as patches, elements in (c, py, px) order.
//
// Shape: fit_resize_u8_kernel's. A workgroup owns CP_TH rows x CP_TW pixels
// of the crop, one lane one channel column of it; the source rows the tile
// needs pass through LDS in chunks of CP_ROWS (horizontal pass into LDS,
// vertical pass out of it into CP_TH f32 registers). Tap loops are sized
// from the scale at run time: any H, W runs, no tap is truncated. The
// rounded tile is staged in LDS and leaves with px along the lanes, so a
// lane run writes whole 14-element patch rows.
// ---------------------------------------------------------------------------
#define CP_TW 64
#define CP_TH 8
#define CP_COLS (CP_TW * 3)
#define CP_ROWS 32

// Keys cubic, a = -0.5
__device__ __forceinline__ float cubic_weight(float x) {
  x = fabsf(x);
  if (x < 1.0f) return (1.5f * x - 2.5f) * x * x + 1.0f;
  if (x < 2.0f) return ((-0.5f * x + 2.5f) * x - 4.0f) * x + 2.0f;
  return 0.0f;
}

__global__ __launch_bounds__(CP_COLS) void clip_patches_kernel(
    const f16* __restrict__ img, f16* __restrict__ out,
    const f16* __restrict__ lut, int H, int W, int size, int patch, int nh,
    int nw, int top, int left) {
  __shared__ float rows[CP_ROWS * CP_COLS];
  const int tid = threadIdx.x;
  const int col = blockIdx.x * CP_COLS + tid;  // channel column of the crop
  const int px = col / 3, chn = col - px * 3;
  const int ty0 = blockIdx.y * CP_TH;
  const bool col_ok = col < size * 3;
  const f16* src = img + (long)blockIdx.z * H * W * 3;

  const double sx = (double)W / nw, sy = (double)H / nh;
  const double fsx = fmax(sx, 1.0), fsy = fmax(sy, 1.0);
  const float iscx = (float)(1.0 / fsx), iscy = (float)(1.0 / fsy);

  // horizontal taps of this lane's pixel: xs.., xn taps, fx = xs - c + 0.5
  int xs = 0, xn = 0;
  float fx = 0.0f, inv_nx = 0.0f;
  if (col_ok) {
    int xe;
    double c;
    fit_taps(px + left, sx, 2.0 * fsx, W, xs, xe, c);
    xn = xe - xs;
    fx = (float)(xs - c + 0.5);
    float sum = 0.0f;
    for (int k = 0; k < xn; ++k) sum += cubic_weight((fx + k) * iscx);
    inv_nx = 1.0f / sum;
  }

  // vertical taps of the tile's rows (block-uniform); rows past the crop keep
  // zero taps and are never written
  int ys[CP_TH], ye[CP_TH];
  float dy[CP_TH], inv_ny[CP_TH], acc[CP_TH];
  int ylo = 0, yhi = 0;
  bool any = false;
#pragma unroll
  for (int t = 0; t < CP_TH; ++t) {
    ys[t] = ye[t] = 0;
    dy[t] = inv_ny[t] = acc[t] = 0.0f;
    if (ty0 + t < size) {
      double c;
      fit_taps(ty0 + t + top, sy, 2.0 * fsy, H, ys[t], ye[t], c);
      if (!any) ylo = ys[t];
      any = true;
      yhi = ye[t];
      // weight argument (r - c + 0.5) == (r - ylo) - dy
      dy[t] = (float)(c - 0.5 - ylo);
      float sum = 0.0f;
      for (int r = ys[t]; r < ye[t]; ++r)
        sum += cubic_weight(((float)(r - ylo) - dy[t]) * iscy);
      inv_ny[t] = 1.0f / sum;
    }
  }

  for (int r0 = ylo; r0 < yhi; r0 += CP_ROWS) {
    const int nr = min(CP_ROWS, yhi - r0);
    if (col_ok) {
      // r0 + r < yhi <= H and xs + k < xs + xn <= W
      const f16* base = src + ((long)r0 * W + xs) * 3 + chn;
      for (int r = 0; r < nr; ++r) {
        const f16* p = base + (long)r * W * 3;
        float a = 0.0f;
        for (int k = 0; k < xn; ++k)
          a += cubic_weight((fx + k) * iscx) * (float)post_u8(p[k * 3]);
        rows[r * CP_COLS + tid] = a * inv_nx;
      }
    }
    __syncthreads();
    if (col_ok) {
#pragma unroll
      for (int t = 0; t < CP_TH; ++t) {
        const int a = max(ys[t], r0), b = min(ye[t], r0 + nr);
        for (int r = a; r < b; ++r)
          acc[t] += cubic_weight(((float)(r - ylo) - dy[t]) * iscy) *
                    rows[(r - r0) * CP_COLS + tid];
      }
    }
    __syncthreads();
  }

  // the last __syncthreads() of the chunk loop released `rows`
  uint8_t* tile = reinterpret_cast<uint8_t*>(rows);
#pragma unroll
  for (int t = 0; t < CP_TH; ++t) {
    float v = nearbyintf(acc[t] * inv_ny[t]);
    v = fminf(255.0f, fmaxf(0.0f, v));
    tile[t * CP_COLS + tid] = col_ok ? (uint8_t)v : 0;
  }
  __syncthreads();
  const int grid = size / patch, pp = patch * patch;
  f16* dst = out + (long)blockIdx.z * grid * grid * 3 * pp;
  for (int i = tid; i < CP_TH * CP_COLS; i += CP_COLS) {
    const int t = i / CP_COLS, rem = i - t * CP_COLS;
    const int c = rem / CP_TW, lx = rem - c * CP_TW;
    const int y = ty0 + t, x = blockIdx.x * CP_TW + lx;
    if (y < size && x < size) {
      const int gy = y / patch, gx = x / patch;
      const long o = ((long)(gy * grid + gx) * 3 + c) * pp +
                     (y - gy * patch) * patch + (x - gx * patch);
      dst[o] = lut[c * 256 + tile[t * CP_COLS + lx * 3 + c]];
    }
  }
}

extern "C" void airtc_clip_patches(const uint16_t* img, uint16_t* out,
                                   const uint16_t* lut, int B, int H, int W,
                                   int size, int patch, int nh, int nw,
                                   int top, int left, hipStream_t s) {
  dim3 grid((size + CP_TW - 1) / CP_TW, (size + CP_TH - 1) / CP_TH, B);
  hipLaunchKernelGGL(clip_patches_kernel, grid, dim3(CP_COLS), 0, s,
                     reinterpret_cast<const f16*>(img),
                     reinterpret_cast<f16*>(out),
                     reinterpret_cast<const f16*>(lut), H, W, size, patch, nh,
                     nw, top, left);
}

// ---------------------------------------------------------------------------
// quick_gelu (f16, vec8, f32 math): x * sigmoid(1.702 x) as one division
// ---------------------------------------------------------------------------
__global__ void quick_gelu_kernel(const f16* __restrict__ in,
                                  f16* __restrict__ out, long n8) {
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += gridDim.x * blockDim.x) {
    f16x8 v = reinterpret_cast<const f16x8*>(in)[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = (float)v[j];
      v[j] = (f16)(x / (1.0f + expf(-1.702f * x)));
    }
    reinterpret_cast<f16x8*>(out)[i] = v;
  }
}

extern "C" void airtc_quick_gelu_f16(const uint16_t* in, uint16_t* out, long n,
                                     hipStream_t s) {
  long n8 = n / 8;
  int blocks = (int)min((long)EW_MAX_BLOCKS, (n8 + EW_BLOCK - 1) / EW_BLOCK);
  if (blocks < 1) return;
  hipLaunchKernelGGL(quick_gelu_kernel, dim3(blocks), dim3(EW_BLOCK), 0, s,
                     reinterpret_cast<const f16*>(in),
                     reinterpret_cast<f16*>(out), n8);
}

// ---------------------------------------------------------------------------
// safety_head: one workgroup per frame, everything after the tower.
//   y      = LayerNorm(cls) * g + b                         (f32)
//   e      = proj_w (proj x hidden, f16) . y                (f32 accumulation)
//   cos_r  = (e . table_r) / |e|     table rows unit-norm f32, special first
//   special_j = cos_j - special_w_j + adj
//   care      = 0.01 if any(special_j > 0) else 0
//   concept_i = cos_i - concept_w_i + adj + care
//   flag      = any(concept_i > 0);  counters[b] += flag
// Nothing is rounded to f16 between the LayerNorm and the scores. y, e and
// the cosines live in dynamic LDS: (hidden + proj + ns + nc + 4) floats. One
// writer per flags / scores / counters element: plain stores.
// ---------------------------------------------------------------------------
#define HEAD_BLOCK 256
#define HEAD_WAVES (HEAD_BLOCK / WAVE)

__device__ __forceinline__ float head_block_sum(float v, float* red) {
  v = wave_reduce(v, SumOp());
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  float total = 0.0f;
#pragma unroll
  for (int w = 0; w < HEAD_WAVES; ++w) total += red[w];
  __syncthreads();  // red may be written again
  return total;
}

__global__ __launch_bounds__(HEAD_BLOCK) void safety_head_kernel(
    const f16* __restrict__ cls, long cls_stride,
    const float* __restrict__ ln_g, const float* __restrict__ ln_b,
    const f16* __restrict__ proj_w, const float* __restrict__ special,
    const float* __restrict__ special_w, const float* __restrict__ concept,
    const float* __restrict__ concept_w, const float* __restrict__ adjust,
    int* __restrict__ counters, int* __restrict__ flags,
    float* __restrict__ scores, int hidden, int proj, int ns, int nc,
    float eps) {
  // one dynamic region, no static LDS in front of it
  extern __shared__ float head_lds[];
  float* y = head_lds;          // hidden
  float* e = y + hidden;        // proj
  float* cosv = e + proj;       // ns + nc
  float* red = cosv + ns + nc;  // HEAD_WAVES
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int b = blockIdx.x;
  const f16* x = cls + (long)b * cls_stride;

  // LayerNorm, two passes over the LDS copy
  float part = 0.0f;
  for (int i = tid * 8; i < hidden; i += HEAD_BLOCK * 8) {
    const f16x8 v = *reinterpret_cast<const f16x8*>(x + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      y[i + j] = (float)v[j];
      part += (float)v[j];
    }
  }
  const float mean = head_block_sum(part, red) / hidden;
  part = 0.0f;
  for (int i = tid; i < hidden; i += HEAD_BLOCK) {
    const float d = y[i] - mean;
    part += d * d;
  }
  const float rstd = 1.0f / sqrtf(head_block_sum(part, red) / hidden + eps);
  for (int i = tid; i < hidden; i += HEAD_BLOCK)
    y[i] = (y[i] - mean) * rstd * ln_g[i] + ln_b[i];
  __syncthreads();

  // projection: a wave per output row, 8 columns per lane per step
  for (int r = wave; r < proj; r += HEAD_WAVES) {
    const f16* wrow = proj_w + (long)r * hidden;
    float acc = 0.0f;
    for (int i = lane * 8; i < hidden; i += WAVE * 8) {
      const f16x8 w = *reinterpret_cast<const f16x8*>(wrow + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += (float)w[j] * y[i + j];
    }
    acc = wave_reduce(acc, SumOp());
    if (lane == 0) e[r] = acc;
  }
  __syncthreads();

  part = 0.0f;
  for (int i = tid; i < proj; i += HEAD_BLOCK) part += e[i] * e[i];
  const float inv_norm = 1.0f / sqrtf(head_block_sum(part, red));

  const int nt = ns + nc;
  for (int r = wave; r < nt; r += HEAD_WAVES) {
    const float* trow = r < ns ? special + (long)r * proj
                               : concept + (long)(r - ns) * proj;
    float acc = 0.0f;
    for (int i = lane; i < proj; i += WAVE) acc += e[i] * trow[i];
    acc = wave_reduce(acc, SumOp());
    if (lane == 0) cosv[r] = acc * inv_norm;
  }
  __syncthreads();

  if (tid == 0) {
    const float adj = adjust[b];
    float* sc = scores + (long)b * nt;
    bool care = false;
    for (int j = 0; j < ns; ++j) {
      const float v = cosv[j] - special_w[j] + adj;
      sc[j] = v;
      care = care || v > 0.0f;
    }
    const float lift = care ? 0.01f : 0.0f;
    int flag = 0;
    for (int i = 0; i < nc; ++i) {
      const float v = cosv[ns + i] - concept_w[i] + adj + lift;
      sc[ns + i] = v;
      flag |= v > 0.0f ? 1 : 0;
    }
    flags[b] = flag;
    counters[b] += flag;
  }
}

extern "C" int airtc_safety_head_lds_bytes(int hidden, int proj, int ns,
                                           int nc) {
  return (hidden + proj + ns + nc + HEAD_WAVES) * (int)sizeof(float);
}

extern "C" void airtc_safety_head(
    const uint16_t* cls, long cls_stride, const float* ln_g,
    const float* ln_b, const uint16_t* proj_w, const float* special,
    const float* special_w, const float* concept, const float* concept_w,
    const float* adjust, int* counters, int* flags, float* scores, int B,
    int hidden, int proj, int ns, int nc, float eps, hipStream_t s) {
  hipLaunchKernelGGL(safety_head_kernel, dim3(B), dim3(HEAD_BLOCK),
                     airtc_safety_head_lds_bytes(hidden, proj, ns, nc), s,
                     reinterpret_cast<const f16*>(cls), cls_stride, ln_g, ln_b,
                     reinterpret_cast<const f16*>(proj_w), special, special_w,
                     concept, concept_w, adjust, counters, flags, scores,
                     hidden, proj, ns, nc, eps);
}

// ---------------------------------------------------------------------------
// blank_flagged: frames whose flag is set become -1 everywhere, in place;
// the others are not written. per = elements per frame; vec != 0: per % 8
// == 0 and img 16-byte aligned (the caller checks).
// ---------------------------------------------------------------------------
__global__ void blank_flagged_kernel(f16* __restrict__ img,
                                     const int* __restrict__ flags, long per,
                                     int vec) {
  if (flags[blockIdx.y] == 0) return;
  f16* p = img + (long)blockIdx.y * per;
  const long start = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long step = (long)gridDim.x * blockDim.x;
  if (vec) {
    f16x8 m;
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = (f16)-1.0f;
    for (long i = start; i < per / 8; i += step)
      reinterpret_cast<f16x8*>(p)[i] = m;
  } else {
    for (long i = start; i < per; i += step) p[i] = (f16)-1.0f;
  }
}

extern "C" void airtc_blank_flagged(uint16_t* img, const int* flags, int B,
                                    long per, int vec, hipStream_t s) {
  const long n = vec ? per / 8 : per;
  int blocks = (int)min((long)256, (n + EW_BLOCK - 1) / EW_BLOCK);
  if (blocks < 1 || B < 1) return;
  hipLaunchKernelGGL(blank_flagged_kernel, dim3(blocks, B), dim3(EW_BLOCK), 0,
                     s, reinterpret_cast<f16*>(img), flags, per, vec);
}
