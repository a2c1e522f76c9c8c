// Per-row LoRA delta for batched serving (gfx950):
//
//   y[b, :, col : col+N] += scale[b] * (x[b] . A[a]^T) . B[a]^T,  a = adapter[b]
//
// x (Bt, L, K), y (Bt, L, Ny), A (n, R, K) "down", B (n, N, R) "up", all f16;
// adapter (Bt,) i32 and scale (Bt,) f32 are read on the device, so a captured
// graph follows a table rewritten under it. A row with adapter[b] < 0 costs
// its workgroups one 4-byte read: they return before any load of x, A, B, y.
//
// One workgroup of four waves owns 16 tokens of one row and a contiguous
// share of the N/16 output tiles. Both products are mfma_f32_16x16x32_f16:
//
//  1. tT = A[a] . xT, R/16 accumulator tiles of (16 r, 16 tokens). The four
//     waves take every fourth 32-wide k-step each and add their partial
//     accumulators through LDS (f32, fixed order), so x and A[a] are read
//     once per workgroup and every wave then holds all of tT. The A
//     operand is A[a] (r on l&15, k = 8(l>>4)+j: one 16-byte load), the B
//     operand is x (token on l&15, same k: one 16-byte load). Lane l ends up
//     with tT[r = 16c + 4(l>>4) + i][token = l&15], i = 0..3, per tile c.
//  2. yT = B[a] . tT. tT's accumulators, rounded to f16, ARE the B operand:
//     the token is already on l&15 and the sum runs over r, the register
//     index. The k order inside a 32-step is then permuted: element j of lane
//     quarter h = l>>4 is r = 32s + 16(j>>2) + 4h + (j&3), so B[a]'s fragment
//     takes its element j from that same r: two 8-byte loads. R = 16 fills
//     only j < 4; the upper half of both operands is zero.
//     Lane l gets yT[n = 4(l>>4) + i][token = l&15]: four consecutive columns
//     of one token, one 8-byte read-modify-write of y. The workgroup's output
//     tiles go round the four waves.
//
// The scale multiplies the f32 product; the sum with y rounds to f16 once.
#include "common.h"
#include "kernels.h"

typedef __attribute__((__vector_size__(4 * sizeof(_Float16)))) _Float16 f16x4;

namespace {

constexpr int LORA_WAVES = 4;

template <int RC>  // R / 16
__global__ __launch_bounds__(LORA_WAVES* WAVE) void lora_delta_kernel(
    const f16* __restrict__ x, f16* __restrict__ y, const f16* __restrict__ A,
    const f16* __restrict__ Bw, const int* __restrict__ row_adapter,
    const float* __restrict__ row_scale, int L, int K, int N, int Ny,
    int col_offset, int n_adapters, int ltiles, int nsplit) {
  constexpr int R = RC * 16;
  constexpr int KS2 = (RC + 1) / 2;  // 32-wide k-steps of the second product
  const int b = blockIdx.z;
  const int a = row_adapter[b];
  // workgroup-uniform: nothing of x, A, B, y is touched for a bare row. An
  // index past the bank is a bare row too, never an out-of-bounds read.
  if (a < 0 || a >= n_adapters) return;
  const float scale = row_scale[b];

  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  const int lt = blockIdx.x % ltiles, split = blockIdx.x / ltiles;
  const int ntiles = N >> 4;
  const int per = (ntiles + nsplit - 1) / nsplit;
  const int nt0 = split * per, nt1 = min(nt0 + per, ntiles);
  if (nt0 >= nt1) return;  // workgroup-uniform as well: before the barrier

  const int l15 = lane & 15, h = lane >> 4;
  const int tok = lt * 16 + l15;
  const bool live = tok < L;
  // a token past L reads the row's last one (in bounds) and stores nothing
  const f16* xp = x + ((size_t)b * L + (live ? tok : L - 1)) * K + 8 * h;
  const f16* ap = A + ((size_t)a * R + l15) * K + 8 * h;

  f32x4 acc[RC];
#pragma unroll
  for (int c = 0; c < RC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = wave * 32; k0 < K; k0 += LORA_WAVES * 32) {
    const f16x8 xf = *reinterpret_cast<const f16x8*>(xp + k0);
#pragma unroll
    for (int c = 0; c < RC; ++c) {
      const f16x8 af =
          *reinterpret_cast<const f16x8*>(ap + (size_t)c * 16 * K + k0);
      acc[c] = mfma16x16x32(af, xf, acc[c]);
    }
  }

  // sum the waves' partial products: every wave ends with the whole tT
  __shared__ f32x4 part[LORA_WAVES][RC][WAVE];
#pragma unroll
  for (int c = 0; c < RC; ++c) part[wave][c][lane] = acc[c];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < RC; ++c) {
    acc[c] = part[0][c][lane];
#pragma unroll
    for (int w = 1; w < LORA_WAVES; ++w) acc[c] += part[w][c][lane];
  }

  // the intermediate, rounded to f16 once, in the second product's k order
  f16x8 tf[KS2];
#pragma unroll
  for (int s = 0; s < KS2; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = 2 * s + (j >> 2);
      tf[s][j] = c < RC ? (f16)acc[c < RC ? c : 0][j & 3] : (f16)0.f;
    }

  const f16* bp = Bw + ((size_t)a * N + l15) * R + 4 * h;
  f16* yp = y + ((size_t)b * L + tok) * Ny + col_offset + 4 * h;
  for (int nt = nt0 + wave; nt < nt1; nt += LORA_WAVES) {
    f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS2; ++s) {
      const f16* p = bp + (size_t)nt * 16 * R + 32 * s;
      const f16x4 lo = *reinterpret_cast<const f16x4*>(p);
      f16x4 hi = f16x4{(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
      if (2 * s + 1 < RC) hi = *reinterpret_cast<const f16x4*>(p + 16);
      const f16x8 bf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      d = mfma16x16x32(bf, tf[s], d);
    }
    if (live) {
      f16x4* q = reinterpret_cast<f16x4*>(yp + nt * 16);
      const f16x4 y0 = *q;
      f16x4 r;
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = (f16)((float)y0[i] + scale * d[i]);
      *q = r;
    }
  }
}

}  // namespace

extern "C" int airtc_lora_delta(const uint16_t* x, uint16_t* y,
                                const uint16_t* A, const uint16_t* B,
                                const int* row_adapter, const float* row_scale,
                                int Bt, int L, int K, int N, int Ny, int R,
                                int col_offset, int n_adapters,
                                hipStream_t s) {
  if (Bt < 1 || Bt > 65535 || L < 1 || K < 32 || K % 32 || N < 16 || N % 16 ||
      col_offset < 0 || col_offset % 16 || col_offset + N > Ny || Ny % 4 ||
      n_adapters < 1 || (R != 16 && R != 32 && R != 64))
    return -1;
  const int ltiles = ceil_div(L, 16), ntiles = N / 16;
  // recomputing the first product is cheaper than idle CUs: split the output
  // tiles over more workgroups until about two waves per SIMD exist, as long
  // as each wave keeps an output tile or more
  int nsplit = 1;
  while ((long)ltiles * nsplit * Bt * LORA_WAVES < 2048 &&
         ntiles / (nsplit * 2) >= LORA_WAVES)
    nsplit *= 2;
  const long blocks = (long)ltiles * nsplit;
  dim3 grid((unsigned)blocks, 1, (unsigned)Bt), block(LORA_WAVES * WAVE);
  const f16* xf = reinterpret_cast<const f16*>(x);
  f16* yf = reinterpret_cast<f16*>(y);
  const f16* Af = reinterpret_cast<const f16*>(A);
  const f16* Bf = reinterpret_cast<const f16*>(B);
#define LORA_LAUNCH(RC)                                                      \
  hipLaunchKernelGGL(lora_delta_kernel<RC>, grid, block, 0, s, xf, yf, Af,   \
                     Bf, row_adapter, row_scale, L, K, N, Ny, col_offset,    \
                     n_adapters, ltiles, nsplit)
  if (R == 16)
    LORA_LAUNCH(1);
  else if (R == 32)
    LORA_LAUNCH(2);
  else
    LORA_LAUNCH(4);
#undef LORA_LAUNCH
  return 0;
}
