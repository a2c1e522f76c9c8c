// YUV 4:2:0 colour conversion: packed u8 RGB <-> planar I420, and the
// engine's f16 postprocess fused with RGB -> I420.
//
// An I420 frame is (3H/2, W) u8, H and W even: H*W bytes of Y, then
// (H/2)*(W/2) of Cb, then (H/2)*(W/2) of Cr, all tight. The arithmetic is
// the software codec's (h264sw.cpp rgb_to_yuv420_rows / yuv420_to_rgb):
// BT.601 limited range in integers, chroma from the rounded 2x2 RGB mean on
// the way out and nearest-replicated on the way in, so every result is
// bit-exact against the codec and the torch reference.
//
// Shape: one lane owns a 2-row x 8-column block = four chroma samples.
// Out: 24 B (u8) or 48 B (f16) of wide loads per row, one 8 B Y store per
// row and one 4 B store to each of Cb and Cr. In: the mirror image. Lanes of
// a wave own consecutive column blocks, so the Y/Cb/Cr accesses are
// lane-contiguous and the three RGB accesses of a row together cover whole
// lines. A block that is narrower than 8 columns (W % 8 != 0) or whose
// addresses the wide accesses cannot take aligned (odd pitches, offset
// bases) runs the scalar 2x2 path in the same launch. Every access stays
// inside the planes for any even H, W >= 2 (the host side rejects the rest).

#include <algorithm>

#include "common.h"
#include "yuv_math.h"

#define YUV_BLOCK 64  // 512x512 is 16384 lanes: one wave per CU
#define YUV_MAX_BLOCKS 4096

namespace {

// one 2x2 quad: p = {r,g,b} of (row0,x) (row0,x+1) (row1,x) (row1,x+1)
__device__ __forceinline__ void quad_to_yuv(const uint8_t p[12], uint8_t y[4],
                                            uint8_t& cb, uint8_t& cr) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    y[k] = luma_of(p[3 * k], p[3 * k + 1], p[3 * k + 2]);
  const int R = (p[0] + p[3] + p[6] + p[9] + 2) >> 2;
  const int G = (p[1] + p[4] + p[7] + p[10] + 2) >> 2;
  const int B = (p[2] + p[5] + p[8] + p[11] + 2) >> 2;
  chroma_of(R, G, B, cb, cr);
}

// clip8(v >> 8). The empty asm keeps the shift and the clamp apart: fused,
// the compiler packs pairs of them into v_ashr_pk_u8_i32, and on the MI355X
// a dword assembled from that result came out with a stray bit above the
// two packed bytes (a G value one too high next to a saturated R).
__device__ __forceinline__ uint8_t shr8_clip8(int v) {
  v >>= 8;
  asm volatile("" : "+v"(v));
  return clip8(v);
}

__device__ __forceinline__ void yuv_to_rgb(int y, int cb, int cr,
                                           uint8_t* rgb) {
  const int C = y - 16, D = cb - 128, E = cr - 128;
  rgb[0] = shr8_clip8(298 * C + 409 * E + 128);
  rgb[1] = shr8_clip8(298 * C - 100 * D - 208 * E + 128);
  rgb[2] = shr8_clip8(298 * C + 516 * D + 128);
}

// source element -> u8: identity, or postprocess_u8_kernel's expression
__device__ __forceinline__ uint8_t src_u8(uint8_t v) { return v; }
__device__ __forceinline__ uint8_t src_u8(f16 v) {
  float f = ((float)v + 1.0f) * 127.5f;
  return (uint8_t)min(255.0f, max(0.0f, nearbyintf(f)));
}

// 24 consecutive source elements (8 RGB pixels) -> u8, wide loads
__device__ __forceinline__ void load_row24(const uint8_t* p, uint8_t o[24]) {
  const uint2* q = reinterpret_cast<const uint2*>(p);
  uint2 v[3] = {q[0], q[1], q[2]};
  const uint8_t* b = reinterpret_cast<const uint8_t*>(v);
#pragma unroll
  for (int j = 0; j < 24; ++j) o[j] = b[j];
}
__device__ __forceinline__ void load_row24(const f16* p, uint8_t o[24]) {
  const f16x8* q = reinterpret_cast<const f16x8*>(p);
  f16x8 v[3] = {q[0], q[1], q[2]};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) o[8 * k + j] = src_u8(v[k][j]);
}

__device__ __forceinline__ bool is_aligned(const void* p, unsigned a) {
  return ((uintptr_t)p & (a - 1)) == 0;
}

// (B,H,W,3) T -> (B,3H/2,W) u8 I420; T = u8 RGB or f16 in [-1,1]
template <typename T>
__global__ __launch_bounds__(YUV_BLOCK) void to_i420_kernel(
    const T* __restrict__ in, uint8_t* __restrict__ out, int B, int H, int W) {
  const int wb = (W + 7) >> 3, hb = H >> 1, cw = W >> 1;
  const long plane = (long)H * W, frame = plane + plane / 2;
  const long total = (long)B * hb * wb;
  // wide-load alignment: 3 x 8 B (u8) or 3 x 16 B (f16) per row
  const unsigned la = sizeof(T) == 1 ? 8 : 16;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int xb = (int)(i % wb);
    const long r = i / wb;
    const int yb = (int)(r % hb);
    const long b = r / hb;
    const int x0 = xb << 3, y0 = yb << 1;
    const int n = min(8, W - x0);  // columns of this block (even, >= 2)
    const T* p0 = in + ((b * H + y0) * W + x0) * 3;
    const T* p1 = p0 + (long)W * 3;
    uint8_t* oy0 = out + b * frame + (long)y0 * W + x0;
    uint8_t* oy1 = oy0 + W;
    uint8_t* ocb = out + b * frame + plane + (long)yb * cw + (x0 >> 1);
    uint8_t* ocr = ocb + plane / 4;
    if (n == 8 && is_aligned(p0, la) && is_aligned(p1, la) &&
        is_aligned(oy0, 8) && is_aligned(oy1, 8) && is_aligned(ocb, 4) &&
        is_aligned(ocr, 4)) {
      uint8_t a[24], c[24];
      load_row24(p0, a);
      load_row24(p1, c);
      uint2 ya, yc;
      uint32_t vb, vr;
      uint8_t* y0b = reinterpret_cast<uint8_t*>(&ya);
      uint8_t* y1b = reinterpret_cast<uint8_t*>(&yc);
      uint8_t* cbb = reinterpret_cast<uint8_t*>(&vb);
      uint8_t* crb = reinterpret_cast<uint8_t*>(&vr);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint8_t p[12], y[4];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          p[j] = a[6 * q + j];
          p[6 + j] = c[6 * q + j];
        }
        quad_to_yuv(p, y, cbb[q], crb[q]);
        y0b[2 * q] = y[0];
        y0b[2 * q + 1] = y[1];
        y1b[2 * q] = y[2];
        y1b[2 * q + 1] = y[3];
      }
      *reinterpret_cast<uint2*>(oy0) = ya;
      *reinterpret_cast<uint2*>(oy1) = yc;
      *reinterpret_cast<uint32_t*>(ocb) = vb;
      *reinterpret_cast<uint32_t*>(ocr) = vr;
    } else {
      for (int q = 0; q < (n >> 1); ++q) {
        uint8_t p[12], y[4], cb, cr;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          p[j] = src_u8(p0[6 * q + j]);
          p[6 + j] = src_u8(p1[6 * q + j]);
        }
        quad_to_yuv(p, y, cb, cr);
        oy0[2 * q] = y[0];
        oy0[2 * q + 1] = y[1];
        oy1[2 * q] = y[2];
        oy1[2 * q + 1] = y[3];
        ocb[q] = cb;
        ocr[q] = cr;
      }
    }
  }
}

// (B,3H/2,W) u8 I420 -> (B,H,W,3) u8 RGB
__global__ __launch_bounds__(YUV_BLOCK) void i420_to_rgb_kernel(
    const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int B, int H,
    int W) {
  const int wb = (W + 7) >> 3, hb = H >> 1, cw = W >> 1;
  const long plane = (long)H * W, frame = plane + plane / 2;
  const long total = (long)B * hb * wb;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int xb = (int)(i % wb);
    const long r = i / wb;
    const int yb = (int)(r % hb);
    const long b = r / hb;
    const int x0 = xb << 3, y0 = yb << 1;
    const int n = min(8, W - x0);
    const uint8_t* iy0 = in + b * frame + (long)y0 * W + x0;
    const uint8_t* iy1 = iy0 + W;
    const uint8_t* icb = in + b * frame + plane + (long)yb * cw + (x0 >> 1);
    const uint8_t* icr = icb + plane / 4;
    uint8_t* o0 = out + ((b * H + y0) * W + x0) * 3;
    uint8_t* o1 = o0 + (long)W * 3;
    if (n == 8 && is_aligned(iy0, 8) && is_aligned(iy1, 8) &&
        is_aligned(icb, 4) && is_aligned(icr, 4) && is_aligned(o0, 8) &&
        is_aligned(o1, 8)) {
      const uint2 ya = *reinterpret_cast<const uint2*>(iy0);
      const uint2 yc = *reinterpret_cast<const uint2*>(iy1);
      const uint32_t vb = *reinterpret_cast<const uint32_t*>(icb);
      const uint32_t vr = *reinterpret_cast<const uint32_t*>(icr);
      const uint8_t* y0b = reinterpret_cast<const uint8_t*>(&ya);
      const uint8_t* y1b = reinterpret_cast<const uint8_t*>(&yc);
      const uint8_t* cbb = reinterpret_cast<const uint8_t*>(&vb);
      const uint8_t* crb = reinterpret_cast<const uint8_t*>(&vr);
      uint2 ra[3], rc[3];
      uint8_t* a = reinterpret_cast<uint8_t*>(ra);
      uint8_t* c = reinterpret_cast<uint8_t*>(rc);
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        yuv_to_rgb(y0b[x], cbb[x >> 1], crb[x >> 1], a + 3 * x);
        yuv_to_rgb(y1b[x], cbb[x >> 1], crb[x >> 1], c + 3 * x);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        reinterpret_cast<uint2*>(o0)[k] = ra[k];
        reinterpret_cast<uint2*>(o1)[k] = rc[k];
      }
    } else {
      for (int x = 0; x < n; ++x) {
        const int cb = icb[x >> 1], cr = icr[x >> 1];
        yuv_to_rgb(iy0[x], cb, cr, o0 + 3 * x);
        yuv_to_rgb(iy1[x], cb, cr, o1 + 3 * x);
      }
    }
  }
}

int yuv_grid(int B, int H, int W) {
  const long total = (long)B * (H / 2) * ((W + 7) / 8);
  return (int)std::max(
      1L, std::min((long)YUV_MAX_BLOCKS, (total + YUV_BLOCK - 1) / YUV_BLOCK));
}

}  // namespace

extern "C" void airtc_rgb_u8_to_i420(const uint8_t* in, uint8_t* out, int B,
                                     int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(to_i420_kernel<uint8_t>, dim3(yuv_grid(B, H, W)),
                     dim3(YUV_BLOCK), 0, s, in, out, B, H, W);
}

extern "C" void airtc_postprocess_i420(const uint16_t* in, uint8_t* out, int B,
                                       int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(to_i420_kernel<f16>, dim3(yuv_grid(B, H, W)),
                     dim3(YUV_BLOCK), 0, s, reinterpret_cast<const f16*>(in),
                     out, B, H, W);
}

extern "C" void airtc_i420_to_rgb_u8(const uint8_t* in, uint8_t* out, int B,
                                     int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(i420_to_rgb_kernel, dim3(yuv_grid(B, H, W)),
                     dim3(YUV_BLOCK), 0, s, in, out, B, H, W);
}
