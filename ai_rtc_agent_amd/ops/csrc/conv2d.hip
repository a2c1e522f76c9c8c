// Conv2d NHWC — implicit-GEMM on MFMA (CDNA4 16x16x32 f16 tiles).
//
// MI355X-native replacement for the reference's TensorRT UNet/VAE conv
// engines (reference lib/wrapper.py:409-512).
// One MFMA schedule (register-staged, single LDS buffer, 2 barriers per
// K-step) in four instantiations; the schedules that measured slower or
// neutral are retired (profiles/optimization_ladder.md, "Retired
// experiments"). Designed for gfx950:
//
//  - GEMM view M=(HO·WO) pixels x N=OC x K=R·S·IC; the im2col gather runs
//    on the fly with INLINE zero-padding (per-load bounds predicate — no
//    padded input copy, no aten F.pad fill+copy kernels)
//  - channel runs are 16B-contiguous (IC%32==0 on the MFMA path): each lane
//    stages 8 f16 per load (guide G13)
//  - LDS tiles padded by one 16B access width (guide G4) for ds_read_b128
//  - T14 async-stage split: next K-tile's global loads issue before the
//    current tile's MFMAs
//  - EPILOGUE FUSION: bias + per-(batch,channel) bias (time-embedding add)
//    + residual add + activation, all in the conv store
//  - two tile geometries + SPLIT-K: the UNet's small-spatial wide-channel
//    layers (8²x1280: M=64, K=11520) would otherwise launch 20 workgroups
//    on a 256-CU chip (measured 235us each, 56% of frame time); split-K
//    over the K loop with f32 slab partials + a finalize pass fills the
//    chip (profiles/ has the before/after)
//
// Geometry A (large M): BM=128 BN=64, 4 waves (2x2), wave=64x32, 8 MFMA/step
// Geometry B (small M): BM=64  BN=64, 4 waves (2x2), wave=32x32, 4 MFMA/step
// Both take split-K over blockIdx.z; the rest of the file is the split-K
// finalize kernels and the tiny-IC / small-IC / direct kernels for
// IC % 32 != 0.
//
// Operands read where they lie (no kernel whose only job is to move them):
//  - SECOND K SEGMENT: an optional second A source x2 (B, HO, WO, IC2), read
//    as a 1x1 stride-1 tap at the output pixel by the K-tiles past R*S*IC
//    against one packed (OC, R*S*IC + IC2) weight — a resnet's 1x1 shortcut
//    inside conv2's K loop. The source is picked per K-tile (block-uniform)
//    in load_tile; split-K and the finalize only see a longer K.
//  - NEAREST-2X IN THE A-LOAD: bounds against the upsampled extents, address
//    (hi>>1, wi>>1) on the half-size source. Bit-identical to upsample +
//    conv.
//    Both are compile-time modes of conv2d_mfma_kernel (third template
//    parameter): as runtime arguments they cost ~5 % on every plain conv.
//  - TINY IC (IC <= 4, the 4-channel conv_in layers): conv2d_tinyic_kernel,
//    lanes along OC, weights in registers, pixels as LDS broadcasts,
//    coalesced 128 B stores, no scratch.

#include <stdlib.h>

#include "common.h"
#include "kernels.h"

#define BN 64

struct KPos {
  int r, s, ic0;
};

__device__ __forceinline__ KPos kpos_at(int k0, int IC, int S) {
  const int rs = k0 / IC;
  return {rs / S, rs - (rs / S) * S, k0 - rs * IC};
}

// one staged 16B A-load with inline zero-padding. aff (optional,
// per-channel float pairs pre-offset for the batch) applies the fused
// GroupNorm affine + activation AT LOAD TIME — the producing GN-apply
// kernel and a full activation HBM round-trip disappear. Padding lanes
// stay zero (ok-gated): the transform models act(gn(x)) of the unfused
// pipeline, which the conv then zero-pads.
// UP (0/1, compile time): the conv reads a nearest-2x upsampled view of its
// source. H, W are the extents the conv sees (bounds check); the source is
// (H>>1, W>>1) and the tap's address is (hi>>1, wi>>1) — a shift in the
// address, no arithmetic on the data, same values in the same K order as a
// materialised upsample.
template <int UP>
__device__ __forceinline__ f16x8 load_a(const f16* xb, int ho_s, int wo_s,
                                        int r, int s, int pad, int H, int W,
                                        int IC, int ic, const float* aff,
                                        int in_act) {
  const int hi = ho_s + r - pad;
  const int wi = wo_s + s - pad;
  const bool ok = (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W;
  const int hc = ok ? hi >> UP : 0, wc = ok ? wi >> UP : 0;
  f16x8 v = *reinterpret_cast<const f16x8*>(
      &xb[((long)hc * (W >> UP) + wc) * IC + ic]);
  if (!ok) {
    v = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
  } else if (aff) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = (float)v[j] * aff[(ic + j) * 2] + aff[(ic + j) * 2 + 1];
      v[j] = (f16)apply_act(f, in_act);
    }
  }
  return v;
}

// fused epilogue value: acc + bias + cbias, + residual, then act
__device__ __forceinline__ f16 epilogue(float acc, const float* bias,
                                        const f16* cbias, long cb_off,
                                        const f16* residual, long idx, int oc,
                                        int act) {
  float v = acc;
  if (bias) v += bias[oc];
  if (cbias) v += (float)cbias[cb_off + oc];
  if (residual) v += (float)residual[idx];
  return (f16)apply_act(v, act);
}

// ---------------------------------------------------------------------------
// templated MFMA conv: MFRAG = M-fragments per wave (4 -> BM=128, 2 -> BM=64)
// BK = K-tile depth: 64 when IC%64==0 (all SD/TAESD layers — halves the
// barrier count per K element, 2 MFMA K-chunks per stage), else 32.
// splitk = number of K splits (>= 1) carried in blockIdx.z next to the
// batch; splitk > 1: partials go to ws (f32), the finalize pass reduces.
// Schedule: register-staged, single LDS buffer, two barriers per K-step.
// MODE selects how the A operand is addressed. It is a template parameter
// and not a kernel argument because the runtime form (a variable shift in
// load_a, a branch in load_tile) measured ~5 % on EVERY conv of the frame;
// MODE 0 compiles to the plain kernel.
//  CONV_PLAIN: x only.
//  CONV_TAIL:  x2/IC2 is a second K segment, a (B, HO, WO, IC2) tensor read
//    as a 1x1 stride-1 unpadded tap at the output pixel. w rows are
//    [R*S*IC | IC2] long (K = R*S*IC + IC2) and K-tiles past R*S*IC stage
//    their A chunk from x2 — the choice is per K-tile, block-uniform, made
//    in load_tile. Needs stride == 1 and IC2 % BK == 0 (host-checked).
//    in_aff applies to segment 0 only.
//  CONV_UP:    nearest-2x source addressing of x (load_a<1>): x is
//    (B, H/2, W/2, IC), H and W stay the extents the conv sees.
// ---------------------------------------------------------------------------
enum { CONV_PLAIN = 0, CONV_TAIL = 1, CONV_UP = 2 };

template <int MFRAG, int BK, int MODE>
__global__ __launch_bounds__(256) void conv2d_mfma_kernel(
    const f16* __restrict__ x, const f16* __restrict__ w,
    const float* __restrict__ bias, const f16* __restrict__ cbias,
    const f16* __restrict__ residual, f16* __restrict__ out,
    float* __restrict__ ws, int H, int W, int IC, int HO, int WO, int OC,
    int R, int S, int stride, int pad, int act, int K, int splitk,
    const float* __restrict__ in_aff, int in_act,
    const f16* __restrict__ x2, int IC2) {
  constexpr int UP = MODE == CONV_UP ? 1 : 0;
  constexpr int BM = MFRAG * 32;              // 128 or 64
  constexpr int NFRAG = BN / 32;              // N-fragments per wave
  constexpr int KPITCH = BK + 8;              // +16B row pad (guide G4)
  constexpr int ALOADS = MFRAG * BK / 64;     // staged 16B A-loads per thread
  constexpr int BLOADS = NFRAG * BK / 64;     // staged 16B B-loads per thread
  constexpr int KSH = BK == 64 ? 3 : 2;       // flat -> (row, k8) shifts
  constexpr int KMSK = BK / 8 - 1;
  __shared__ f16 ldsA[BM * KPITCH];
  __shared__ f16 ldsB[BN * KPITCH];

  const int M = HO * WO;
  const int n_tiles = ceil_div_dev(OC, BN);
  const int mt = blockIdx.x / n_tiles;
  const int nt = blockIdx.x - mt * n_tiles;
  const int m0 = mt * BM;
  const int n0 = nt * BN;
  const int b = blockIdx.z / splitk;
  const int split = blockIdx.z - b * splitk;
  const f16* xb = x + (long)b * (H >> UP) * (W >> UP) * IC;
  const float* affb = in_aff ? in_aff + (long)b * IC * 2 : nullptr;
  const int K1 = K - IC2;                     // end of the conv segment
  const f16* x2b = x2 + (long)b * M * IC2;    // used only when IC2 > 0

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid & 1;
  const int wn = wid >> 1;

  // staging map
  int a_row[ALOADS], a_ho[ALOADS], a_wo[ALOADS], a_k8[ALOADS];
#pragma unroll
  for (int i = 0; i < ALOADS; ++i) {
    int flat = tid + i * 256;           // [0, BM*BK/8)
    a_row[i] = flat >> KSH;
    a_k8[i] = (flat & KMSK) * 8;
    int m = min(m0 + a_row[i], M - 1);
    a_ho[i] = (m / WO) * stride;
    a_wo[i] = (m % WO) * stride;
  }
  int b_row[BLOADS], b_k8[BLOADS];
  const f16* wrow[BLOADS];
#pragma unroll
  for (int i = 0; i < BLOADS; ++i) {
    int flat = tid + i * 256;           // [0, BN*BK/8)
    b_row[i] = flat >> KSH;
    b_k8[i] = (flat & KMSK) * 8;
    wrow[i] = w + (long)min(n0 + b_row[i], OC - 1) * K + b_k8[i];
  }

  f32x4 acc[MFRAG][NFRAG];
#pragma unroll
  for (int mi = 0; mi < MFRAG; ++mi)
#pragma unroll
    for (int ni = 0; ni < NFRAG; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

  // K-step range for this split
  const int nk = K / BK;
  const int per = (nk + splitk - 1) / splitk;
  const int k_lo = split * per;
  const int k_hi = min(nk, k_lo + per);
  // NOTE: an empty split (uneven tail) still stores its zero slab below —
  // the finalize pass reads every slab.

  // staging helpers
  f16x8 regA[ALOADS], regB[BLOADS];
  auto load_tile = [&](int kt) {
    const int k0 = kt * BK;
    if (MODE != CONV_TAIL || k0 < K1) {
      KPos p = kpos_at(k0, IC, S);
#pragma unroll
      for (int i = 0; i < ALOADS; ++i)
        regA[i] = load_a<UP>(xb, a_ho[i], a_wo[i], p.r, p.s, pad, H, W, IC,
                             p.ic0 + a_k8[i], affb, in_act);
    } else {
      // pointwise tail: stride 1, so a_ho/a_wo are the output pixel itself
      const f16* t = x2b + (k0 - K1);
#pragma unroll
      for (int i = 0; i < ALOADS; ++i) {
        // the pixel offset is loop-invariant; recomputing it per tail tile
        // from a_ho/a_wo (opaque to the optimiser) keeps it from being
        // hoisted into ALOADS extra live registers across the main K loop
        int ho = a_ho[i];
        asm volatile("" : "+v"(ho));
        regA[i] = *reinterpret_cast<const f16x8*>(
            &t[(ho * WO + a_wo[i]) * IC2 + a_k8[i]]);
      }
    }
#pragma unroll
    for (int i = 0; i < BLOADS; ++i)
      regB[i] = *reinterpret_cast<const f16x8*>(wrow[i] + kt * BK);
  };
  auto write_tile = [&]() {
#pragma unroll
    for (int i = 0; i < ALOADS; ++i)
      *reinterpret_cast<f16x8*>(&ldsA[a_row[i] * KPITCH + a_k8[i]]) = regA[i];
#pragma unroll
    for (int i = 0; i < BLOADS; ++i)
      *reinterpret_cast<f16x8*>(&ldsB[b_row[i] * KPITCH + b_k8[i]]) = regB[i];
  };
  const int arow_base = wm * (MFRAG * 16) + (lane & 15);
  auto compute_tile = [&]() {
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      const int fcol = kk * 32 + (lane >> 4) * 8;
      f16x8 bfrag[NFRAG];
#pragma unroll
      for (int ni = 0; ni < NFRAG; ++ni)
        bfrag[ni] = *reinterpret_cast<const f16x8*>(
            &ldsB[(wn * (NFRAG * 16) + ni * 16 + (lane & 15)) * KPITCH + fcol]);
#pragma unroll
      for (int mi = 0; mi < MFRAG; ++mi) {
        f16x8 afrag = *reinterpret_cast<const f16x8*>(
            &ldsA[(arow_base + mi * 16) * KPITCH + fcol]);
#pragma unroll
        for (int ni = 0; ni < NFRAG; ++ni)
          acc[mi][ni] = mfma16x16x32(afrag, bfrag[ni], acc[mi][ni]);
      }
    }
  };

  // 2-barrier single-buffer loop (T14 prefetch only)
  if (k_lo < k_hi) load_tile(k_lo);
  for (int kt = k_lo; kt < k_hi; ++kt) {
    __syncthreads();
    write_tile();
    __syncthreads();
    if (kt + 1 < k_hi) load_tile(kt + 1);
    compute_tile();
  }

  if (splitk == 1) {
    f16* ob = out + (long)b * M * OC;
    const long cb_off = (long)b * OC;
#pragma unroll
    for (int ni = 0; ni < NFRAG; ++ni) {
      const int col = n0 + wn * (NFRAG * 16) + ni * 16 + (lane & 15);
      if (col >= OC) continue;
#pragma unroll
      for (int mi = 0; mi < MFRAG; ++mi)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int m = m0 + wm * (MFRAG * 16) + mi * 16 + (lane >> 4) * 4 + j;
          if (m < M) {
            const long idx = (long)b * M * OC + (long)m * OC + col;
            ob[(long)m * OC + col] = epilogue(acc[mi][ni][j], bias, cbias,
                                              cb_off, residual, idx, col, act);
          }
        }
    }
  } else {
    // f32 slab store; the finalize pass reduces the slabs and applies the
    // epilogue
    float* wsb = ws + ((long)b * splitk + split) * M * OC;
#pragma unroll
    for (int ni = 0; ni < NFRAG; ++ni) {
      const int col = n0 + wn * (NFRAG * 16) + ni * 16 + (lane & 15);
      if (col >= OC) continue;
#pragma unroll
      for (int mi = 0; mi < MFRAG; ++mi)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int m = m0 + wm * (MFRAG * 16) + mi * 16 + (lane >> 4) * 4 + j;
          if (m < M) wsb[(long)m * OC + col] = acc[mi][ni][j];
        }
    }
  }
}

__global__ void conv_splitk_finalize(const float* __restrict__ ws,
                                     const float* __restrict__ bias,
                                     const f16* __restrict__ cbias,
                                     const f16* __restrict__ residual,
                                     f16* __restrict__ out, int M, int OC,
                                     int splitk, int act, long total) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * (long)blockDim.x) {
    const int oc = i % OC;
    const long bm = i / OC;
    const long b = bm / M;
    const float* p = ws + (long)b * splitk * M * OC + (bm - b * M) * OC + oc;
    float a = 0.f;
    for (int s = 0; s < splitk; ++s) a += p[(long)s * M * OC];
    out[i] = epilogue(a, bias, cbias, b * OC, residual, i, oc, act);
  }
}

// Vectorized finalize (OC % 4 == 0). A block is CT column lanes x PT pixel
// rows (PT = 256 / CT): each lane owns 4 consecutive output channels of one
// column tile and walks the block's pixel range, so pixel and column are
// derived once per thread and the loop only advances pointers. Per pixel:
// one 16 B f32 load per slab, 8 B bias/cbias/residual loads, one 8 B f16
// store. Grid = (pixel chunks, column tiles, B). The epilogue law and order
// are the scalar kernel's: act(sum_s slab + bias + cbias + residual).
//
// STATS: the column tile is a whole number of GroupNorm groups (CT*4 ==
// gpt*Cg) and the block also emits this pixel chunk's per-group sum / sumsq
// of the ROUNDED f16 outputs into `part` ([B*G][gridDim.x][2], the layout in
// kernels.h) — the consumer's stats pass disappears. Fixed-order register /
// LDS reduction, one writer per slot: deterministic, no atomics, no fence.
typedef __attribute__((__vector_size__(4 * sizeof(_Float16)))) _Float16 f16x4;

template <bool STATS>
__global__ __launch_bounds__(256) void conv_splitk_finalize_v4(
    const float* __restrict__ ws, const float* __restrict__ bias,
    const f16* __restrict__ cbias, const f16* __restrict__ residual,
    f16* __restrict__ out, float* __restrict__ part, int M, int OC,
    int splitk, int act, int ct, int per, int Cg, int G) {
  const int cx = threadIdx.x % ct, py = threadIdx.x / ct;
  const int pt = 256 / ct;
  const int cw = ct * 4;
  const int b = blockIdx.z;
  const int c0 = blockIdx.y * cw + cx * 4;
  const int p_lo = blockIdx.x * per;
  const int p_hi = min(M, p_lo + per);
  float s4[4] = {0.f, 0.f, 0.f, 0.f}, q4[4] = {0.f, 0.f, 0.f, 0.f};
  if (py < pt && c0 < OC) {
    f32x4 bv = {0.f, 0.f, 0.f, 0.f}, cv = {0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + c0);
    if (cbias) {
      const f16x4 c = *reinterpret_cast<const f16x4*>(cbias + (long)b * OC + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) cv[j] = (float)c[j];
    }
    const long slab = (long)M * OC;
    const long o = ((long)b * M + p_lo + py) * OC + c0;
    const float* wp = ws + (long)b * splitk * slab + (long)(p_lo + py) * OC + c0;
    const f16* rp = residual ? residual + o : nullptr;
    f16* op = out + o;
    const long step = (long)pt * OC;
    for (int p = p_lo + py; p < p_hi; p += pt) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int s = 0; s < splitk; ++s)
        a += *reinterpret_cast<const f32x4*>(wp + (long)s * slab);
      if (bias) a += bv;
      if (cbias) a += cv;
      if (rp) {
        const f16x4 r = *reinterpret_cast<const f16x4*>(rp);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += (float)r[j];
        rp += step;
      }
      f16x4 h;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h[j] = (f16)apply_act(a[j], act);
        if (STATS) {
          const float f = (float)h[j];
          s4[j] += f;
          q4[j] += f * f;
        }
      }
      *reinterpret_cast<f16x4*>(op) = h;
      wp += step;
      op += step;
    }
  }
  if (STATS) {
    // pt * cw <= 1024 and cw <= 128 (host plan)
    __shared__ float red[2][1024];
    __shared__ float col[2][128];
    if (py < pt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        red[0][py * cw + cx * 4 + j] = s4[j];
        red[1][py * cw + cx * 4 + j] = q4[j];
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < cw) {
      float a0 = 0.f, a1 = 0.f;
      for (int r = 0; r < pt; ++r) {
        a0 += red[0][r * cw + threadIdx.x];
        a1 += red[1][r * cw + threadIdx.x];
      }
      col[0][threadIdx.x] = a0;
      col[1][threadIdx.x] = a1;
    }
    __syncthreads();
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
}

// ---------------------------------------------------------------------------
// Small-IC conv (ragged IC < 32; the 3/4-channel conv_in layers now take
// conv2d_tinyic_kernel below): one thread per output PIXEL computing
// a 64-wide OC tile in registers, weights staged once in LDS (uniform k ->
// broadcast reads). The one-thread-per-output direct kernel re-reads each
// input pixel OC times (measured 169us for TAESD conv_in @512²); this reads
// x once per pixel (~14 MB total) and streams the output.
// ---------------------------------------------------------------------------
#define OCT 64
#define SMALLIC_MAX_K 288  // 3x3 x IC<32

__global__ __launch_bounds__(256) void conv2d_smallic_kernel(
    const f16* __restrict__ x, const f16* __restrict__ w,
    const float* __restrict__ bias, const f16* __restrict__ cbias,
    const f16* __restrict__ residual, f16* __restrict__ out, int H, int W,
    int IC, int HO, int WO, int OC, int R, int S, int stride, int pad,
    int act, int K, long total_pix, const float* __restrict__ in_aff,
    int in_act) {
  __shared__ f16 wlds[SMALLIC_MAX_K * OCT];
  const int oc0 = blockIdx.y * OCT;
  for (int i = threadIdx.x; i < K * OCT; i += 256) {
    const int k = i / OCT, oc = i - (i / OCT) * OCT;
    wlds[i] = (oc0 + oc < OC) ? w[(long)(oc0 + oc) * K + k] : (f16)0;
  }
  __syncthreads();

  const int M = HO * WO;
  const int noc = min(OCT, OC - oc0);
  for (long pix = blockIdx.x * (long)blockDim.x + threadIdx.x; pix < total_pix;
       pix += gridDim.x * (long)blockDim.x) {
    const int m = pix % M;
    const long b = pix / M;
    const int ho = m / WO, wo = m % WO;
    const f16* xb = x + b * (long)H * W * IC;
    const float* affb = in_aff ? in_aff + b * (long)IC * 2 : nullptr;
    float acc[OCT];
#pragma unroll
    for (int o = 0; o < OCT; ++o) acc[o] = 0.f;
    for (int r = 0; r < R; ++r) {
      const int hi = ho * stride + r - pad;
      if ((unsigned)hi >= (unsigned)H) continue;
      for (int s = 0; s < S; ++s) {
        const int wi = wo * stride + s - pad;
        if ((unsigned)wi >= (unsigned)W) continue;
        const f16* xr = &xb[((long)hi * W + wi) * IC];
        const f16* wr = &wlds[(r * S + s) * IC * OCT];
        for (int c = 0; c < IC; ++c) {
          float xv = (float)xr[c];
          if (affb)
            xv = apply_act(xv * affb[c * 2] + affb[c * 2 + 1], in_act);
          const f16* wv = &wr[c * OCT];
#pragma unroll
          for (int o = 0; o < OCT; ++o) acc[o] += xv * (float)wv[o];
        }
      }
    }
    const long obase = (b * M + m) * (long)OC + oc0;
    const long cb_off = b * OC;
    for (int o = 0; o < noc; ++o)
      out[obase + o] = epilogue(acc[o], bias, cbias, cb_off, residual,
                                obase + o, oc0 + o, act);
  }
}

// ---------------------------------------------------------------------------
// Tiny-IC conv (the 4- and 3-channel conv_in layers, K = R*S*IC <= 36):
// lanes along OC. A wave owns one 64-wide OC tile: each lane keeps its
// output channel's K weights in registers (read coalesced from a (TK, OC)
// f32 pack built once per weight, rows past K zero) and the block's pixels
// are staged as zero-padded f32 im2col rows in LDS, read back as wave-uniform
// broadcasts. Per pixel a wave issues TK FMAs per lane and ONE coalesced
// 128 B f16 store — against the per-pixel kernel above there are no 64
// accumulators per thread (no scratch) and no strided 2 B stores, and the
// grid is pixel chunks x OC tiles (>= 2 blocks per CU at 64²: ppb is sized
// by the host). Accumulation order is (r, s, c) ascending in f32, as above.
// ---------------------------------------------------------------------------
#define TINY_TK 36    // 3x3 x IC<=4
#define TINY_PPB 64   // max pixels per block

__global__ __launch_bounds__(256) void conv2d_tinyic_kernel(
    const f16* __restrict__ x, const float* __restrict__ wt,
    const float* __restrict__ bias, const f16* __restrict__ cbias,
    const f16* __restrict__ residual, f16* __restrict__ out, int H, int W,
    int IC, int HO, int WO, int OC, int S, int stride, int pad, int act,
    int K, long total_pix, int ppb) {
  __shared__ __attribute__((aligned(16))) float xs[TINY_PPB * TINY_TK];
  const long pix0 = blockIdx.x * (long)ppb;
  const int npix = (int)min((long)ppb, total_pix - pix0);
  const int M = HO * WO;
  // im2col rows of this block's pixels, zero where padded or past K
  for (int i = threadIdx.x; i < npix * TINY_TK; i += 256) {
    const int p = i / TINY_TK, k = i - p * TINY_TK;
    float v = 0.f;
    if (k < K) {
      const long pix = pix0 + p;
      const long b = pix / M;
      const int m = (int)(pix - b * M);
      const int ho = m / WO, wo = m - ho * WO;
      const int rs = k / IC, c = k - rs * IC;
      const int r = rs / S, s = rs - r * S;
      const int hi = ho * stride + r - pad, wi = wo * stride + s - pad;
      if ((unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W)
        v = (float)x[((b * H + hi) * (long)W + wi) * IC + c];
    }
    xs[i] = v;
  }
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int oc = blockIdx.y * 64 + lane;
  const bool live = oc < OC;
  float wr[TINY_TK];
#pragma unroll
  for (int k = 0; k < TINY_TK; ++k) wr[k] = live ? wt[(long)k * OC + oc] : 0.f;
  const float bv = (bias && live) ? bias[oc] : 0.f;
  __syncthreads();
  for (int p = wid; p < npix; p += 4) {
    const f32x4* xr = reinterpret_cast<const f32x4*>(&xs[p * TINY_TK]);
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < TINY_TK / 4; ++q) {
      const f32x4 xv = xr[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) a += xv[j] * wr[q * 4 + j];
    }
    if (live) {
      const long pix = pix0 + p;
      const long b = pix / M;
      const long idx = pix * OC + oc;
      float v = a;
      if (bias) v += bv;
      if (cbias) v += (float)cbias[b * OC + oc];
      if (residual) v += (float)residual[idx];
      out[idx] = (f16)apply_act(v, act);
    }
  }
}

// ---------------------------------------------------------------------------
// Direct conv fallback (ragged shapes the other kernels exclude)
// ---------------------------------------------------------------------------
__global__ void conv2d_direct_kernel(
    const f16* __restrict__ x, const f16* __restrict__ w,
    const float* __restrict__ bias, const f16* __restrict__ cbias,
    const f16* __restrict__ residual, f16* __restrict__ out, int H, int W,
    int IC, int HO, int WO, int OC, int R, int S, int stride, int pad, int act,
    int K, long total, const float* __restrict__ in_aff, int in_act) {
  const int M = HO * WO;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * (long)blockDim.x) {
    const int oc = i % OC;
    long rest = i / OC;
    const int m = rest % M;
    const long b = rest / M;
    const int ho = m / WO, wo = m % WO;
    const f16* xb = x + b * (long)H * W * IC;
    const float* affb = in_aff ? in_aff + b * (long)IC * 2 : nullptr;
    const f16* wk = w + (long)oc * K;
    float a = 0.f;
    for (int r = 0; r < R; ++r) {
      const int hi = ho * stride + r - pad;
      if ((unsigned)hi >= (unsigned)H) continue;
      for (int s = 0; s < S; ++s) {
        const int wi = wo * stride + s - pad;
        if ((unsigned)wi >= (unsigned)W) continue;
        const f16* xr = &xb[((long)hi * W + wi) * IC];
        const f16* wr = &wk[(r * S + s) * IC];
        for (int c = 0; c < IC; ++c) {
          float xv = (float)xr[c];
          if (affb)
            xv = apply_act(xv * affb[c * 2] + affb[c * 2 + 1], in_act);
          a += xv * (float)wr[c];
        }
      }
    }
    out[i] = epilogue(a, bias, cbias, b * OC, residual, i, oc, act);
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
extern "C" int airtc_conv2d_splitk_for(int B, int HO, int WO, int OC, int IC) {
  // path/geometry decision, exported so the host can size the workspace:
  // returns 0 = direct, +k = BM128 split-K k, -k = BM64 split-K k.
  // Target ~2 blocks/CU (>=480 workgroups): at 1 block/CU a wave can only
  // hide latency with its own ILP (measured: 64x64x320 conv at 160 blocks
  // ran 87us = 86 TF; split-K over the K loop fills the chip).
  if (IC % 32 != 0) return 0;
  const int M = HO * WO;
  if (M >= 2048) {
    const long blocks = (long)ceil_div(M, 128) * ceil_div(OC, BN) * B;
    long k = (480 + blocks - 1) / blocks;
    if (k < 1) k = 1;
    if (k > 8) k = 8;
    return (int)k;
  }
  const long blocks64 = (long)ceil_div(M, 64) * ceil_div(OC, BN) * B;
  long k = (512 + blocks64 - 1) / blocks64;
  if (k < 1) k = 1;
  if (k > 32) k = 32;
  return (int)(-k);
}

// A/B switch: AIRTC_FIN_VEC=0 keeps the scalar finalize (and with it no
// fused statistics)
static int conv_fin_vec() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("AIRTC_FIN_VEC");
    v = (e && atoi(e) == 0) ? 0 : 1;
  }
  return v;
}
// GroupNorm statistics from the finalize are opt-in (AIRTC_FIN_STATS=1):
// measured NEUTRAL end-to-end on MI355X (146.9/148.2/147.1 fps with them vs
// 147.8/147.2 without, same session, under the hipGraph): the 43 stats
// launches they remove are paid back by the slower stats-emitting finalize
// at 64x64 and by an apply that inherits the finalize's smaller chunk count.
// Read per call so one process can run both.
static int conv_fin_stats() {
  const char* e = getenv("AIRTC_FIN_STATS");
  return conv_fin_vec() && e && atoi(e) == 1;
}

// geometry of the vectorized finalize: ct column lanes (4 channels each),
// per pixels per block, nchunk pixel chunks
struct FinPlan { int ct, per, nchunk; };

// stats variant: column tile = gpt whole groups (<= 128 channels, a multiple
// of 4), nchunk <= 64 pixel chunks with no empty chunk
static bool fin_stats_plan(int M, int OC, int G, FinPlan* p) {
  if (G <= 0 || OC % 4 != 0 || OC % G != 0) return false;
  const int Cg = OC / G;
  if (Cg & 1) return false;
  int gpt = 0;
  for (int d = 1; d <= G; ++d)
    if (G % d == 0 && d * Cg <= 128 && (d * Cg) % 4 == 0) gpt = d;
  if (!gpt) return false;
  p->ct = gpt * Cg / 4;
  const int pt = 256 / p->ct;
  const int n0 = min(64, ceil_div(M, pt));
  p->per = ceil_div(M, n0);
  p->nchunk = ceil_div(M, p->per);
  return true;
}

extern "C" int airtc_conv2d_stats_nchunk(int B, int HO, int WO, int OC, int IC,
                                         int G, int act) {
  const int path = airtc_conv2d_splitk_for(B, HO, WO, OC, IC);
  const int splitk = path > 0 ? path : -path;
  if (splitk < 2) return 0;  // direct path or split = 1: no finalize pass
  if (act != ACT_NONE || !conv_fin_stats()) return 0;
  if (B > 65535) return 0;  // finalize_v4 carries the batch in gridDim.z
  FinPlan p;
  return fin_stats_plan(HO * WO, OC, G, &p) ? p.nchunk : 0;
}

extern "C" int airtc_conv2d_mfma(const AirtcConvArgs* a, hipStream_t s) {
  const int B = a->B, H = a->H, W = a->W, IC = a->IC, HO = a->HO, WO = a->WO,
            OC = a->OC, R = a->R, S = a->S, stride = a->stride, pad = a->pad,
            act = a->act, path = a->path, in_act = a->in_act, IC2 = a->IC2,
            up = a->up, gn_groups = a->gn_groups;
  const float* bias = a->bias;
  const float* in_aff = a->in_aff;
  float* ws = a->ws;
  float* gn_part = a->gn_part;
  // w rows are R*S*IC + IC2 long
  const int K = R * S * IC + IC2;
  const f16* xp = reinterpret_cast<const f16*>(a->x);
  const f16* x2p = reinterpret_cast<const f16*>(a->x2);
  const f16* wp = reinterpret_cast<const f16*>(a->w);
  const f16* cb = reinterpret_cast<const f16*>(a->cbias);
  const f16* res = reinterpret_cast<const f16*>(a->residual);
  f16* op = reinterpret_cast<f16*>(a->out);
  const int M = HO * WO;

  const int splitk = path > 0 ? path : -path;
  const int bm = path > 0 ? 128 : 64;
  dim3 grid(ceil_div(M, bm) * ceil_div(OC, BN), 1, B * splitk);
  // split-K: the epilogue operands belong to the finalize pass
  const float* b1 = splitk == 1 ? bias : nullptr;
  const f16* cb1 = splitk == 1 ? cb : nullptr;
  const f16* res1 = splitk == 1 ? res : nullptr;
  // both K segments must be whole K-tiles
  const bool bk64 = (IC % 64 == 0) && (IC2 % 64 == 0);
  if (x2p && up) return -1;  // one addressing mode per launch
#define CONV_LAUNCH(MF, BKV, MD)                                              \
  hipLaunchKernelGGL((conv2d_mfma_kernel<MF, BKV, MD>), grid, dim3(256), 0,   \
                     s, xp, wp, b1, cb1, res1, op, ws, H, W, IC, HO, WO, OC,  \
                     R, S, stride, pad, act, K, splitk, in_aff, in_act, x2p,  \
                     IC2)
#define CONV_GEOM(MD)                                                         \
  do {                                                                        \
    if (path > 0) {                                                           \
      if (bk64) CONV_LAUNCH(4, 64, MD);                                       \
      else CONV_LAUNCH(4, 32, MD);                                            \
    } else {                                                                  \
      if (bk64) CONV_LAUNCH(2, 64, MD);                                       \
      else CONV_LAUNCH(2, 32, MD);                                            \
    }                                                                         \
  } while (0)
  if (x2p) CONV_GEOM(CONV_TAIL);
  else if (up) CONV_GEOM(CONV_UP);
  else CONV_GEOM(CONV_PLAIN);
#undef CONV_GEOM
#undef CONV_LAUNCH
  if (splitk > 1) {
    // 16 B slab / bias loads and 8 B f16 accesses need these alignments
    const uintptr_t al16 = (uintptr_t)ws | (uintptr_t)bias;
    const uintptr_t al8 = (uintptr_t)cb | (uintptr_t)res | (uintptr_t)op;
    const bool vec = conv_fin_vec() && OC % 4 == 0 && (al16 & 15) == 0 &&
                     (al8 & 7) == 0 && B <= 65535;
    FinPlan p;
    if (vec && gn_part && act == ACT_NONE && fin_stats_plan(M, OC, gn_groups, &p)) {
      dim3 fgrid(p.nchunk, OC / (p.ct * 4), B);
      hipLaunchKernelGGL(conv_splitk_finalize_v4<true>, fgrid, dim3(256), 0, s,
                         ws, bias, cb, res, op, gn_part, M, OC, splitk, act,
                         p.ct, p.per, OC / gn_groups, gn_groups);
      return 1;
    } else if (vec) {
      // plain geometry: up to 64 lanes across the channels, ~2048 blocks
      const int oc4 = OC / 4;
      const int ct = min(64, oc4);
      const int tiles = ceil_div(oc4, ct);
      const int pt = 256 / ct;
      const long blocks1 = (long)ceil_div(M, pt) * tiles * B;
      const int ppt = (int)max((long)1, min((long)8, (blocks1 + 2047) / 2048));
      const int per = pt * ppt;
      dim3 fgrid(ceil_div(M, per), tiles, B);
      hipLaunchKernelGGL(conv_splitk_finalize_v4<false>, fgrid, dim3(256), 0,
                         s, ws, bias, cb, res, op, (float*)nullptr, M, OC,
                         splitk, act, ct, per, 0, 0);
    } else {
      long total = (long)B * M * OC;
      int blocks = (int)min((long)2048, (total + 255) / 256);
      hipLaunchKernelGGL(conv_splitk_finalize, dim3(blocks), dim3(256), 0, s,
                         ws, bias, cb, res, op, M, OC, splitk, act, total);
    }
  }
  return 0;
}

extern "C" int airtc_conv2d_tinyic_ok(int IC, int R, int S) {
  return IC <= 4 && R * S * IC <= TINY_TK;
}

extern "C" void airtc_conv2d_tinyic(const AirtcConvArgs* a, hipStream_t s) {
  const long pix = (long)a->B * a->HO * a->WO;
  const int tiles = ceil_div(a->OC, 64);
  // largest pixel chunk that still gives >= 512 blocks (2 per CU), 8..64
  int ppb = TINY_PPB;
  while (ppb > 8 && ((pix + ppb - 1) / ppb) * tiles < 512) ppb >>= 1;
  dim3 grid((uint32_t)((pix + ppb - 1) / ppb), tiles);
  hipLaunchKernelGGL(conv2d_tinyic_kernel, grid, dim3(256), 0, s,
                     reinterpret_cast<const f16*>(a->x),
                     reinterpret_cast<const float*>(a->w), a->bias,
                     reinterpret_cast<const f16*>(a->cbias),
                     reinterpret_cast<const f16*>(a->residual),
                     reinterpret_cast<f16*>(a->out), a->H, a->W, a->IC, a->HO,
                     a->WO, a->OC, a->S, a->stride, a->pad, a->act,
                     a->R * a->S * a->IC, pix, ppb);
}

extern "C" void airtc_conv2d_direct(const AirtcConvArgs* a, hipStream_t s) {
  const f16* x = reinterpret_cast<const f16*>(a->x);
  const f16* w = reinterpret_cast<const f16*>(a->w);
  const f16* cb = reinterpret_cast<const f16*>(a->cbias);
  const f16* res = reinterpret_cast<const f16*>(a->residual);
  f16* out = reinterpret_cast<f16*>(a->out);
  const int K = a->R * a->S * a->IC;
  const long pix = (long)a->B * a->HO * a->WO;
  if (K <= SMALLIC_MAX_K) {
    dim3 grid((uint32_t)min((long)4096, (pix + 255) / 256),
              ceil_div(a->OC, OCT));
    hipLaunchKernelGGL(conv2d_smallic_kernel, grid, dim3(256), 0, s, x, w,
                       a->bias, cb, res, out, a->H, a->W, a->IC, a->HO, a->WO,
                       a->OC, a->R, a->S, a->stride, a->pad, a->act, K, pix,
                       a->in_aff, a->in_act);
    return;
  }
  long total = pix * a->OC;
  int blocks = (int)min((long)4096, (total + 255) / 256);
  hipLaunchKernelGGL(conv2d_direct_kernel, dim3(blocks), dim3(256), 0, s, x, w,
                     a->bias, cb, res, out, a->H, a->W, a->IC, a->HO, a->WO,
                     a->OC, a->R, a->S, a->stride, a->pad, a->act, K, total,
                     a->in_aff, a->in_act);
}
