// Canny edge hint for the ControlNet path: (B,H,W,3) u8 RGB -> (B,H,W,3)
// f16/f32, three equal channels, 1.0 on an edge and 0.0 elsewhere, in ONE
// launch with no global scratch and no host sync.
//
// The operator (ops/interface.py canny_hint_reference is the same arithmetic
// in torch; everything before the final store is integer, so the two agree
// bit for bit):
//   Y  = (77R + 150G + 29B + 128) >> 8
//   S  = (5x5 binomial of Y, taps clamped to the image, + 128) >> 8
//   gx, gy = Sobel 3x3 of S, taps clamped to the image; M = |gx| + |gy|
//   keep = OpenCV's integer-sector non-maximum suppression, M outside the
//          image counting as 0
//   cand = keep && M > low, strong = keep && M > high   (thr[b] = low, high)
//   E0 = strong; `reach` times E <- cand && (3x3 dilation of E)
// The bounded reach (cv2 floods without bound) makes a pixel depend only on
// pixels within Chebyshev distance reach + 4, so a workgroup stages one
// window and never talks to another.
//
// Shape: one 256-thread workgroup per 32x32 output tile and batch row. LDS
// planes, all indexed from the window origin, each 1 px/side smaller than
// the stage before it needs (R = reach):
//   Yp  u8  (32 + 2(R+4))^2   luma, loaded with coordinates clamped to the
//                             image
//   Sp  u8  (32 + 2(R+2))^2   S at clamp(position): an out-of-image entry
//                             holds the S of the nearest image pixel, which
//                             is what a clamped Sobel tap reads (clamp to
//                             the IMAGE edge, never to the window edge)
//   Mp  u16 (32 + 2(R+1))^2   M | sector << 12; 0 outside the image
//   Lp  u8  (32 + 2R)^2       level: 0 strong, k joined in pass k,
//                             254 candidate not yet in, 255 not a candidate
// R = 32 needs 58456 B, R = 16 26712 B, so the default reach keeps several
// workgroups per CU. The propagation runs in place on the level plane: pass
// k admits a waiting candidate next to a level < k; a neighbour admitted in
// the same pass holds k (or still 254), neither of which is < k, so the
// in-place update is the synchronous one. A pass that admits nothing ends
// the loop (every later pass would admit nothing either). Window borders
// lack their outer neighbours; the error moves inward one pixel per pass and
// after R passes has not reached the tile.
//
// The tile is stored as 16-byte chunks at 16-byte-aligned ADDRESSES (the
// rows of an (H,W,3) tensor start anywhere); a chunk that straddles either
// end of the tile's row segment is written element by element, so nothing
// outside out[b, y, x0:x0+n, :] is touched.

#include "common.h"

#define CANNY_TILE 32
#define CANNY_BLOCK 256
#define CANNY_MAX_REACH 32

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

template <typename T> struct CannyOut;
template <> struct CannyOut<f16> {
  typedef f16x8 vec;
  static constexpr int V = 8;
};
template <> struct CannyOut<float> {
  typedef f32x4 vec;
  static constexpr int V = 4;
};

template <typename T>
__global__ __launch_bounds__(CANNY_BLOCK) void canny_hint_kernel(
    const uint8_t* __restrict__ in, const int* __restrict__ thr,
    T* __restrict__ out, int H, int W, int R) {
  extern __shared__ __align__(16) uint8_t canny_smem[];
  const int Wl = CANNY_TILE + 2 * (R + 4);
  const int Ws = CANNY_TILE + 2 * (R + 2);
  const int Wm = CANNY_TILE + 2 * (R + 1);
  const int We = CANNY_TILE + 2 * R;
  uint16_t* Mp = reinterpret_cast<uint16_t*>(canny_smem);
  uint8_t* Yp = canny_smem + Wm * Wm * 2;
  uint8_t* Sp = Yp + Wl * Wl;
  uint8_t* Lp = Sp + Ws * Ws;

  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int ty0 = blockIdx.y * CANNY_TILE, tx0 = blockIdx.x * CANNY_TILE;
  const uint8_t* img = in + (size_t)b * H * W * 3;
  const int low = thr[2 * b], high = thr[2 * b + 1];

  // 1. luma window, coordinates clamped to the image
  for (int i = tid; i < Wl * Wl; i += CANNY_BLOCK) {
    const int wy = i / Wl, wx = i - wy * Wl;
    const int gy = clampi(ty0 - (R + 4) + wy, 0, H - 1);
    const int gx = clampi(tx0 - (R + 4) + wx, 0, W - 1);
    const uint8_t* p = img + ((size_t)gy * W + gx) * 3;
    Yp[i] = (uint8_t)((77 * p[0] + 150 * p[1] + 29 * p[2] + 128) >> 8);
  }
  __syncthreads();

  // 2. S at clamp(position). The clamped position lies between the position
  // and the tile, so it and its +-2 taps are inside the luma window.
  for (int i = tid; i < Ws * Ws; i += CANNY_BLOCK) {
    const int wy = i / Ws, wx = i - wy * Ws;
    const int cy = clampi(ty0 - (R + 2) + wy, 0, H - 1) - (ty0 - (R + 4));
    const int cx = clampi(tx0 - (R + 2) + wx, 0, W - 1) - (tx0 - (R + 4));
    int acc = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
      const uint8_t* row = Yp + (cy + dy) * Wl + cx;
      const int h = row[-2] + 4 * row[-1] + 6 * row[0] + 4 * row[1] + row[2];
      acc += (dy == 0 ? 6 : (dy == -1 || dy == 1) ? 4 : 1) * h;
    }
    Sp[i] = (uint8_t)((acc + 128) >> 8);
  }
  __syncthreads();

  // 3. M and the NMS sector (0 horizontal, 1 vertical, 2 diagonal s = +1,
  // 3 diagonal s = -1); 0 outside the image
  for (int i = tid; i < Wm * Wm; i += CANNY_BLOCK) {
    const int wy = i / Wm, wx = i - wy * Wm;
    const int py = ty0 - (R + 1) + wy, px = tx0 - (R + 1) + wx;
    uint16_t code = 0;
    if (py >= 0 && py < H && px >= 0 && px < W) {
      const uint8_t* s = Sp + (wy + 1) * Ws + (wx + 1);
      const int a = s[-Ws - 1], bb = s[-Ws], c = s[-Ws + 1];
      const int d = s[-1], f = s[1];
      const int g = s[Ws - 1], hh = s[Ws], k = s[Ws + 1];
      const int gx = (c + 2 * f + k) - (a + 2 * d + g);
      const int gy = (g + 2 * hh + k) - (a + 2 * bb + c);
      const int ax = gx < 0 ? -gx : gx, ayv = gy < 0 ? -gy : gy;
      const int M = ax + ayv;  // <= 2040
      const int ay = ayv << 15, t22 = ax * 13573, t67 = t22 + (ax << 16);
      int sector;
      if (ay < t22) sector = 0;
      else if (ay > t67) sector = 1;
      else sector = ((gx ^ gy) < 0) ? 3 : 2;
      code = (uint16_t)(M | (sector << 12));
    }
    Mp[i] = code;
  }
  __syncthreads();

  // 4. non-maximum suppression and classification into the level plane
  for (int i = tid; i < We * We; i += CANNY_BLOCK) {
    const int wy = i / We, wx = i - wy * We;
    const int py = ty0 - R + wy, px = tx0 - R + wx;
    uint8_t lvl = 255;
    if (py >= 0 && py < H && px >= 0 && px < W) {
      const uint16_t* m = Mp + (wy + 1) * Wm + (wx + 1);
      const int code = m[0];
      const int M = code & 0xFFF, sector = code >> 12;
      bool keep;
      if (sector == 0) {
        keep = M > (m[-1] & 0xFFF) && M >= (m[1] & 0xFFF);
      } else if (sector == 1) {
        keep = M > (m[-Wm] & 0xFFF) && M >= (m[Wm] & 0xFFF);
      } else {
        const int s = sector == 2 ? 1 : -1;
        keep = M > (m[-Wm - s] & 0xFFF) && M > (m[Wm + s] & 0xFFF);
      }
      if (keep && M > low) lvl = M > high ? 0 : 254;
    }
    Lp[i] = lvl;
  }
  __syncthreads();

  // 5. bounded-reach hysteresis, in place (see the header)
  for (int k = 1; k <= R; ++k) {
    int changed = 0;
    for (int i = tid; i < We * We; i += CANNY_BLOCK) {
      if (Lp[i] != 254) continue;
      const int wy = i / We, wx = i - wy * We;
      const int y0 = wy > 0 ? -1 : 0, y1 = wy < We - 1 ? 1 : 0;
      const int x0 = wx > 0 ? -1 : 0, x1 = wx < We - 1 ? 1 : 0;
      bool in_reach = false;
      for (int dy = y0; dy <= y1; ++dy)
        for (int dx = x0; dx <= x1; ++dx)
          in_reach |= Lp[i + dy * We + dx] < k;
      if (in_reach) {
        Lp[i] = (uint8_t)k;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }

  // 6. the tile: rows of n pixels = 3n equal-per-pixel elements, as aligned
  // 16-byte chunks
  typedef typename CannyOut<T>::vec vec;
  constexpr int V = CannyOut<T>::V;
  constexpr int CHUNKS = CANNY_TILE * 3 / V + 1;  // a row segment's most
  const int n = min(CANNY_TILE, W - tx0);
  const int rows = min(CANNY_TILE, H - ty0);
  for (int i = tid; i < rows * CHUNKS; i += CANNY_BLOCK) {
    const int r = i / CHUNKS, c = i - r * CHUNKS;
    T* rowp = out + (((size_t)b * H + (ty0 + r)) * W + tx0) * 3;
    const uintptr_t start = reinterpret_cast<uintptr_t>(rowp);
    const uintptr_t addr = (start & ~(uintptr_t)15) + (uintptr_t)c * 16;
    // first element of the chunk relative to the row segment (may be < 0)
    const int e0 = (int)(((intptr_t)addr - (intptr_t)start) / (int)sizeof(T));
    if (e0 >= 3 * n) continue;
    const uint8_t* lrow = Lp + (R + r) * We + R;
    if (e0 >= 0 && e0 + V <= 3 * n) {
      vec v;
#pragma unroll
      for (int j = 0; j < V; ++j)
        v[j] = lrow[(e0 + j) / 3] < 254 ? (T)1.0f : (T)0.0f;
      *reinterpret_cast<vec*>(addr) = v;
    } else {
      for (int j = 0; j < V; ++j) {
        const int e = e0 + j;
        if (e >= 0 && e < 3 * n)
          rowp[e] = lrow[e / 3] < 254 ? (T)1.0f : (T)0.0f;
      }
    }
  }
}

size_t canny_lds_bytes(int R) {
  const size_t Wl = CANNY_TILE + 2 * (R + 4), Ws = CANNY_TILE + 2 * (R + 2);
  const size_t Wm = CANNY_TILE + 2 * (R + 1), We = CANNY_TILE + 2 * R;
  return Wm * Wm * 2 + Wl * Wl + Ws * Ws + We * We;
}

}  // namespace

// in (B,H,W,3) u8, thr (B,2) i32 (low, high) read on the device, out
// (B,H,W,3) f16 (out_f32 == 0) or f32. Returns -1 and launches nothing when
// reach is outside [0, 32] or the grid would not fit.
extern "C" int airtc_canny_hint(const uint8_t* in, const int* thr, void* out,
                                int out_f32, int B, int H, int W, int reach,
                                hipStream_t s) {
  if (reach < 0 || reach > CANNY_MAX_REACH || B < 1 || H < 1 || W < 1)
    return -1;
  const dim3 grid(ceil_div(W, CANNY_TILE), ceil_div(H, CANNY_TILE), B);
  if (grid.y > 65535 || grid.z > 65535) return -1;
  const size_t lds = canny_lds_bytes(reach);
  if (out_f32)
    hipLaunchKernelGGL(canny_hint_kernel<float>, grid, dim3(CANNY_BLOCK), lds,
                       s, in, thr, static_cast<float*>(out), H, W, reach);
  else
    hipLaunchKernelGGL(canny_hint_kernel<f16>, grid, dim3(CANNY_BLOCK), lds, s,
                       in, thr, static_cast<f16*>(out), H, W, reach);
  return 0;
}
