// The package's RGB -> YUV integer arithmetic (BT.601 limited range, the
// software codec's; formulas stated in ops/interface.py), shared by every
// kernel that writes I420 so they stay bit-exact with each other.
#pragma once

#include "common.h"

__device__ __forceinline__ uint8_t clip8(int v) {
  return (uint8_t)min(255, max(0, v));
}

__device__ __forceinline__ uint8_t luma_of(int r, int g, int b) {
  return clip8(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16);
}

// R, G, B: the rounded 2x2 means, (a + b + c + d + 2) >> 2 per channel
__device__ __forceinline__ void chroma_of(int R, int G, int B, uint8_t& cb,
                                          uint8_t& cr) {
  cb = clip8(((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128);
  cr = clip8(((112 * R - 94 * G - 18 * B + 128) >> 8) + 128);
}
