// Fused attention (forward) for ONE WIDE head — d = 512, the AutoencoderKL
// mid-block (heads = 1, width 512, L = H/8 * W/8 tokens).
//
// attention.hip's template keeps a head's whole K and V tile in LDS and its
// whole O row in every wave: at d = 512 that is 133 KB of LDS and 128
// accumulator VGPRs per lane. This kernel splits the HEAD across the
// workgroup instead:
//  - workgroup = 4 waves = ONE 16-row Q tile; grid (ceil(Lq/16), B*H)
//  - kv tile = 64 keys. Wave w computes S for keys 16w..16w+15 over the full
//    d (16 MFMA, Q fragments resident: 64 VGPRs) — K goes global -> VGPR
//    directly in B-fragment shape, no LDS: no other wave reads those keys
//  - the four 16x16 S fragments are exchanged through LDS (f32, [key][q],
//    double-buffered by tile parity: ONE barrier per kv tile)
//  - every wave then runs the SAME online softmax over the 64 keys (so m, l
//    agree bit for bit across waves), writes P to its own transposed bridge
//    tile, and accumulates O for ITS 128 of the 512 output columns: 8
//    fragments = 32 accumulator VGPRs
//  - V: each wave stages only its 64 x 128 column slice, row-major, into a
//    private LDS tile (no barrier: writer = reader) and reads B fragments
//    with ds_read_b64_tr_b16, four fragments per wait (lds_tr.h)
//  - tile t+1's K fragments and V slice are loaded into the SAME registers
//    right after tile t consumed them, ahead of the barrier: the loads fly
//    under t's softmax and PV
// Arithmetic is attention.hip's: base-2 online softmax, m from -1e30, f32
// logits and accumulation, P rounded to f16 for PV only, l sums unrounded P,
// f16 result, Lk tail masked with -1e30.
//
// Budget (D = 512): dynamic LDS 69 632 (V) + 10 240 (S) + 12 288 (P) = 92 160
// B, hence one workgroup per CU and the max-dynamic-shared attribute;
// Q 64 + K 64 + V staging 64 + O 32 VGPRs + softmax temporaries, one wave
// per SIMD.

#include "common.h"
#include "lds_tr.h"

namespace {

constexpr int WKT = 64;  // kv tile
constexpr int WQT = 16;  // q rows per workgroup

template <int D>
struct WideLds {
  static constexpr int DW = D / 4;     // output columns per wave
  static constexpr int VP = DW + 8;    // V pitch (f16): +16 B, as attention.hip
  static constexpr int SP = WQT + 4;   // S pitch (f32), [key][q]
  static constexpr int PP = WQT + 8;   // P bridge pitch (f16), [key][q]
  static constexpr int V_BYTES = 4 * WKT * VP * 2;
  static constexpr int S_BYTES = 2 * WKT * SP * 4;
  static constexpr int P_BYTES = 4 * WKT * PP * 2;
  static constexpr int BYTES = V_BYTES + S_BYTES + P_BYTES;
};

template <int D>
__global__ __launch_bounds__(256) void attention_wide_kernel(
    const f16* __restrict__ q, const f16* __restrict__ k,
    const f16* __restrict__ v, f16* __restrict__ out, int H, int Lq, int Lk,
    long q_sb, long q_sh, long q_row, long k_sb, long k_sh, long k_row,
    long o_sb, long o_sh, long o_row, float scale) {
  using L = WideLds<D>;
  constexpr int KT = WKT;
  constexpr int DW = L::DW, VP = L::VP, SP = L::SP, PP = L::PP;
  constexpr int D32 = D / 32;   // k-steps of S
  constexpr int NFW = DW / 16;  // O fragments per wave
  constexpr int NF = KT / 16;   // S fragments per tile, one per wave
  constexpr int VLOADS = KT * (DW / 8) / 64;  // 16-byte V chunks per lane
  static_assert(D % 128 == 0 && NF == 4 && NFW % 4 == 0, "wide attention tile");
  static_assert(DW / 8 == 16, "V staging maps 16 chunks per row");

  extern __shared__ __attribute__((aligned(16))) unsigned char wide_lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  f16* myV = reinterpret_cast<f16*>(wide_lds) + wid * KT * VP;
  float* ldsS = reinterpret_cast<float*>(wide_lds + L::V_BYTES);
  f16* myP = reinterpret_cast<f16*>(wide_lds + L::V_BYTES + L::S_BYTES) +
             wid * KT * PP;

  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int q0 = blockIdx.x * WQT;
  const int l15 = lane & 15, g = lane >> 4;

  const float scale2 = scale * 1.44269504088896340736f;
  const f16* qb = q + b * q_sb + h * q_sh;
  const f16* kb = k + b * k_sb + h * k_sh;
  const f16* vb = v + b * k_sb + h * k_sh + wid * DW;  // v shares k's layout
  f16* ob = out + b * o_sb + h * o_sh + wid * DW;

  // ---- Q fragments: all 16 rows x D, the same in every wave ----
  f16x8 aq[D32];
  {
    int qrow = q0 + l15;
    if (qrow >= Lq) qrow = Lq - 1;  // never stored
    const f16* qr = qb + (long)qrow * q_row + g * 8;
#pragma unroll
    for (int i = 0; i < D32; ++i)
      aq[i] = *reinterpret_cast<const f16x8*>(qr + i * 32);
  }

  f32x4 o_acc[NFW];
#pragma unroll
  for (int f = 0; f < NFW; ++f) o_acc[f] = {0.f, 0.f, 0.f, 0.f};
  float m_i[4], l_i[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { m_i[j] = -1e30f; l_i[j] = 0.f; }

  // K: this wave's 16 keys as B fragments (lane: key l15, d = 32 i + 8 g ..)
  // V: rows g + 4 i of the wave's column slice, chunk l15
  f16x8 kreg[D32], vreg[VLOADS];
  auto stage_load = [&](int t0) {
    int krow = t0 + wid * 16 + l15;
    if (krow >= Lk) krow = Lk - 1;  // masked in the softmax
    const f16* kr = kb + (long)krow * k_row + g * 8;
#pragma unroll
    for (int i = 0; i < D32; ++i)
      kreg[i] = *reinterpret_cast<const f16x8*>(kr + i * 32);
#pragma unroll
    for (int i = 0; i < VLOADS; ++i) {
      int vrow = t0 + g + i * 4;
      if (vrow >= Lk) vrow = Lk - 1;  // meets P = 0
      vreg[i] = *reinterpret_cast<const f16x8*>(vb + (long)vrow * k_row + l15 * 8);
    }
  };

  stage_load(0);
  int par = 0;
  for (int t0 = 0; t0 < Lk; t0 += KT, par ^= 1) {
    // ---- this wave's S fragment: 16 q x 16 keys over the full d; two
    // accumulators so consecutive MFMAs do not wait on each other ----
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < D32; i += 2) {
      s0 = mfma16x16x32(aq[i], kreg[i], s0);
      s1 = mfma16x16x32(aq[i + 1], kreg[i + 1], s1);
    }
    float* Sb = ldsS + par * KT * SP;
    // C fragment: 4 consecutive q rows of key column l15 -> one 16-byte write
    *reinterpret_cast<f32x4*>(&Sb[(wid * 16 + l15) * SP + g * 4]) = s0 + s1;
    // ---- V slice to the private tile (its last reader, this wave's PV of
    // the previous tile, has completed: every tr read is waited for) ----
#pragma unroll
    for (int i = 0; i < VLOADS; ++i)
      *reinterpret_cast<f16x8*>(&myV[(g + i * 4) * VP + l15 * 8]) = vreg[i];
    if (t0 + KT < Lk) stage_load(t0 + KT);
    // The one barrier per tile: S fragments published. The S buffer of the
    // other parity is rewritten only after the NEXT barrier, which no wave
    // passes before every wave has consumed its reads of this one.
    __syncthreads();

    // ---- online softmax over the tile's 64 keys, identical in all waves ----
    float p[NF][4];
    float mnew[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mnew[j] = -1e30f;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const f32x4 sv =
          *reinterpret_cast<const f32x4*>(&Sb[(nf * 16 + l15) * SP + g * 4]);
      const bool valid = t0 + nf * 16 + l15 < Lk;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float val = valid ? sv[j] * scale2 : -1e30f;
        p[nf][j] = val;
        mnew[j] = fmaxf(mnew[j], val);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mnew[j] = quarter_reduce(mnew[j], MaxOp());
      const float mn = fmaxf(m_i[j], mnew[j]);
      const float alpha = __builtin_amdgcn_exp2f(m_i[j] - mn);
      float rs = 0.f;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        p[nf][j] = __builtin_amdgcn_exp2f(p[nf][j] - mn);
        rs += p[nf][j];
      }
      rs = quarter_reduce(rs, SumOp());
      l_i[j] = l_i[j] * alpha + rs;
      m_i[j] = mn;
#pragma unroll
      for (int f = 0; f < NFW; ++f) o_acc[f][j] *= alpha;
    }
    // ---- P -> this wave's transposed bridge tile [key][q] ----
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      f16x4 pv;
#pragma unroll
      for (int j = 0; j < 4; ++j) pv[j] = (f16)p[nf][j];
      *reinterpret_cast<f16x4*>(&myP[(nf * 16 + l15) * PP + g * 4]) = pv;
    }
    // same-wave LDS write->read: wait for the writes, keep reads below
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- O[:, wave's 128 columns] += P V ----
#pragma unroll
    for (int ks = 0; ks < KT / 32; ++ks) {
      const f16x8 afrag = tr_bfrag(myP, PP, ks * 32, 0, lane);
#pragma unroll
      for (int fb = 0; fb < NFW / 4; ++fb) {
        f16x8 bfrag[4];
        tr_bfrag_x4<VP>(myV, ks * 32, fb * 64, lane, bfrag);
#pragma unroll
        for (int f = 0; f < 4; ++f)
          o_acc[fb * 4 + f] = mfma16x16x32(afrag, bfrag[f], o_acc[fb * 4 + f]);
      }
    }
  }

  // ---- epilogue: O /= l, masked stores ----
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int qrow = q0 + g * 4 + j;
    if (qrow >= Lq) continue;
    const float inv_l = 1.0f / l_i[j];
#pragma unroll
    for (int f = 0; f < NFW; ++f)
      ob[(long)qrow * o_row + f * 16 + l15] = (f16)(o_acc[f][j] * inv_l);
  }
}

}  // namespace

extern "C" int airtc_attention_wide_ok(int d) { return d == 512; }

extern "C" int airtc_attention_wide(const uint16_t* q, const uint16_t* k,
                                    const uint16_t* v, uint16_t* out, int B,
                                    int H, int Lq, int Lk, int d, long q_sb,
                                    long q_sh, long q_row, long k_sb, long k_sh,
                                    long k_row, long o_sb, long o_sh,
                                    long o_row, float scale, hipStream_t s) {
  if (!airtc_attention_wide_ok(d)) return -1;
  constexpr int bytes = WideLds<512>::BYTES;
  auto kern = attention_wide_kernel<512>;
  // more than 64 KB of LDS is opted into per device, once: the first call,
  // which warm-up makes ahead of any graph capture
  static bool opted[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -2;
  if (!opted[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            bytes) != hipSuccess)
      return -3;
    opted[dev] = true;
  }
  dim3 grid(ceil_div(Lq, WQT), B * H);
  hipLaunchKernelGGL(kern, grid, dim3(256), bytes, s,
                     reinterpret_cast<const f16*>(q),
                     reinterpret_cast<const f16*>(k),
                     reinterpret_cast<const f16*>(v),
                     reinterpret_cast<f16*>(out), H, Lq, Lk, q_sb, q_sh, q_row,
                     k_sb, k_sh, k_row, o_sb, o_sh, o_row, scale);
  return 0;
}
