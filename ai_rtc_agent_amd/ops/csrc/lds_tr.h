// gfx950 hardware-transpose LDS reads (ds_read_b64_tr_b16) that turn a
// ROW-major f16 tile into MFMA 16x16x32 operand fragments. Shared by
// attention.hip and attention_wide.hip.
#pragma once

#include "common.h"

typedef __attribute__((__vector_size__(2 * sizeof(unsigned)))) unsigned u32x2;
typedef __attribute__((__vector_size__(4 * sizeof(_Float16)))) _Float16 f16x4;
typedef const __attribute__((address_space(3))) f16* lds_cptr;

__device__ __forceinline__ unsigned lds_addr(const f16* p) {
  return (unsigned)(unsigned long long)(lds_cptr)p;
}

// B-fragment (8 keys x 16 cols) from a ROW-major [kv][pitch] f16 tile via two
// hardware transpose reads. Per 16-lane group g (= keys kbase+8g..+7): lane
// il supplies the address of its 4 contiguous f16 (row kbase+(il>>2),
// col c0+(il&3)*4); the read hands lane il column c0+il over those rows.
// Alignment: addresses are 8B-aligned (pitch even in f16) — required, a
// misaligned tr read returns wrong data silently (guide G17).
__device__ __forceinline__ f16x8 tr_bfrag(const f16* tile, int pitch,
                                          int kbase, int c0, int lane) {
  const int il = lane & 15;
  const int g = lane >> 4;
  const f16* p0 = tile + (kbase + g * 8 + (il >> 2)) * pitch + c0 + (il & 3) * 4;
  const unsigned a0 = lds_addr(p0);
  const unsigned a1 = a0 + 4 * (unsigned)pitch * 2;  // keys +4..+7
  u32x2 lo, hi;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %3\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(lo), "=&v"(hi)
      : "v"(a0), "v"(a1)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);  // rule 18: keep the MFMA below the wait
  union {
    u32x2 u2[2];
    f16x8 f8;
  } cvt;
  cvt.u2[0] = lo;
  cvt.u2[1] = hi;
  return cvt.f8;
}

// Four such fragments, at columns c0, c0+16, c0+32, c0+48 of the same 32
// keys: eight transpose reads in flight behind ONE wait. For a kernel that
// runs one wave per SIMD, where nothing else hides the LDS latency of a
// wait per fragment. PITCH in f16 (compile time: it goes into the
// instructions' offset fields, 4 * PITCH * 2 + 96 < 65536).
template <int PITCH>
__device__ __forceinline__ void tr_bfrag_x4(const f16* tile, int kbase, int c0,
                                            int lane, f16x8 (&out)[4]) {
  static_assert(PITCH % 4 == 0 && 8 * PITCH + 96 < 65536, "tr_bfrag_x4 pitch");
  constexpr int KO = 4 * PITCH * 2;  // bytes to keys +4..+7
  const int il = lane & 15;
  const int g = lane >> 4;
  const f16* p0 = tile + (kbase + g * 8 + (il >> 2)) * PITCH + c0 + (il & 3) * 4;
  const unsigned a0 = lds_addr(p0);
  u32x2 r[8];
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8\n\t"
      "ds_read_b64_tr_b16 %1, %8 offset:%9\n\t"
      "ds_read_b64_tr_b16 %2, %8 offset:32\n\t"
      "ds_read_b64_tr_b16 %3, %8 offset:%10\n\t"
      "ds_read_b64_tr_b16 %4, %8 offset:64\n\t"
      "ds_read_b64_tr_b16 %5, %8 offset:%11\n\t"
      "ds_read_b64_tr_b16 %6, %8 offset:96\n\t"
      "ds_read_b64_tr_b16 %7, %8 offset:%12\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(r[4]),
        "=&v"(r[5]), "=&v"(r[6]), "=&v"(r[7])
      : "v"(a0), "n"(KO), "n"(KO + 32), "n"(KO + 64), "n"(KO + 96)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    union {
      u32x2 u2[2];
      f16x8 f8;
    } cvt;
    cvt.u2[0] = r[2 * f];
    cvt.u2[1] = r[2 * f + 1];
    out[f] = cvt.f8;
  }
}
