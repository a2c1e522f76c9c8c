// Flash-style fused attention (forward) on MFMA — CDNA4 16x16x32 f16.
//
// MI355X-native replacement for the self/cross-attention inside the
// reference's TRT UNet engine. Shapes served:
//   self-attn : Lq = Lk = HW (4096/1024/256/64), d = head_dim (padded to 32)
//   cross-attn: Lk = 77 text tokens
//
// Structure (guide Appendix B "fused attention prefill"):
//  - workgroup = 4 waves = one 64-row Q tile; wave owns 16 q-rows
//  - K/V streamed through LDS in 64-key tiles, BOTH row-major (cheap vec8
//    staging); the PV B-fragment comes out of the row-major V tile via the
//    gfx950 hardware transpose read ds_read_b64_tr_b16 (guide T10) — this
//    replaced a 16-scalar-ds_write-per-thread V transpose at staging
//  - online softmax: running (m, l) per q-row, kept lane-local (each lane
//    owns the same 4 q-rows its C-fragments do), 4x shfl_xor row reduce
//  - P goes through a per-wave LDS tile to convert the C-fragment layout
//    into the A-fragment layout for PV (layout bridge; same-wave, ordered
//    by an lgkmcnt(0) wait, no barrier)
//  - Lk tail masked with -1e30 before the max (cross-attn 77 of 128)
//  - kernel is TEMPLATED on head dim D so every accumulator index is
//    compile-time constant (guide §5.4 rule 20: runtime-indexed vector
//    arrays go to scratch)
//
// Addressing: q/k/v/out are (b, h)-strided views (no host-side copies for
// d%32==0 models; ops/interface.py pads other head sizes).

#include <stdlib.h>

#include "common.h"
#include "lds_tr.h"  // tr_bfrag

#define KVT 64  // kv tile
#define QT 64   // q rows per workgroup

template <int D, int KT = KVT>  // KT = kv tile
__global__ __launch_bounds__(256) void attention_kernel(
    const f16* __restrict__ q, const f16* __restrict__ k,
    const f16* __restrict__ v, f16* __restrict__ out, int H, int Lq, int Lk,
    long q_sb, long q_sh, long q_row, long k_sb, long k_sh, long k_row,
    long o_sb, long o_sh, long o_row, float scale) {
  // q-fragments per wave. 2 (128-row q-tiles) measured slower end to end
  // (profiles/optimization_ladder.md, "Retired experiments").
  constexpr int QF = 1;
  constexpr int KPITCH = D + 8;
  constexpr int D8 = D / 8, D32 = D / 32, D16 = D / 16;
  constexpr int NF = KT / 16;     // 16-key S fragments per tile
  constexpr int QTILE = 64 * QF;  // q rows per workgroup
  // P bridge tile is stored TRANSPOSED [kv][q]: the C-fragment's 4 j-values
  // are 4 consecutive q rows of one kv column, so the write packs into ONE
  // b64 (was 16 scalar f16 writes per (qi, tile)); the PV A-fragment comes
  // back out via the same ds_read_b64_tr_b16 gather the V tile uses.
  constexpr int PT_PITCH = QF * 16 + 8;  // +16B pad: conflict-free b64 law
  __shared__ f16 ldsK[KT * KPITCH];
  __shared__ f16 ldsV[KT * KPITCH];  // row-major like K; PV reads via tr_b16
  __shared__ f16 ldsP[4 * KT * PT_PITCH];

  const int bh = blockIdx.y;
  const int qtile = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int q0 = qtile * QTILE;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;

  // softmax runs in the BASE-2 domain: folding log2(e) into the logit
  // scale turns every exp into a bare v_exp_f32 (exp2) — __expf otherwise
  // pays a v_mul per call, and this kernel is VALU-bound (PMC: 53% busy)
  const float scale2 = scale * 1.44269504088896340736f;
  const f16* qb = q + b * q_sb + h * q_sh;
  const f16* kb = k + b * k_sb + h * k_sh;
  const f16* vb = v + b * k_sb + h * k_sh;  // v shares k's layout
  f16* ob = out + b * o_sb + h * o_sh;

  // ---- Q fragments in registers (one load, reused every kv tile) ----
  f16x8 aq[QF][D32];
#pragma unroll
  for (int qi = 0; qi < QF; ++qi) {
    int qrow = q0 + (wid * QF + qi) * 16 + (lane & 15);
    if (qrow >= Lq) qrow = Lq - 1;
    const f16* qr = qb + (long)qrow * q_row + (lane >> 4) * 8;
#pragma unroll
    for (int i = 0; i < D32; ++i)
      aq[qi][i] = *reinterpret_cast<const f16x8*>(qr + i * 32);
  }

  f32x4 o_acc[QF][D16];
#pragma unroll
  for (int qi = 0; qi < QF; ++qi)
#pragma unroll
    for (int i = 0; i < D16; ++i) o_acc[qi][i] = {0.f, 0.f, 0.f, 0.f};
  float m_i[QF][4], l_i[QF][4];
#pragma unroll
  for (int qi = 0; qi < QF; ++qi)
#pragma unroll
    for (int j = 0; j < 4; ++j) { m_i[qi][j] = -1e30f; l_i[qi][j] = 0.f; }

  f16* myP = &ldsP[wid * KT * PT_PITCH];  // per-wave transposed P tile
  const int fcol = (lane >> 4) * 8;

  // T14 async-stage split: each thread owns LOADS_PT row-chunks of the K and
  // V tiles; tile t+1's global loads are issued right after tile t's LDS
  // image is published, so HBM latency hides under t's MFMA/softmax work.
  constexpr int LOADS_PT = (KT * D8 + 255) / 256;
  f16x8 regK[LOADS_PT], regV[LOADS_PT];
  int st_row[LOADS_PT], st_c8[LOADS_PT];
#pragma unroll
  for (int i = 0; i < LOADS_PT; ++i) {
    const int flat = tid + i * 256;
    st_row[i] = flat / D8;
    st_c8[i] = (flat - st_row[i] * D8) * 8;
  }

  auto stage_load = [&](int t0) {
#pragma unroll
    for (int i = 0; i < LOADS_PT; ++i) {
      if (st_row[i] >= KT) continue;
      int krow = t0 + st_row[i];
      if (krow >= Lk) krow = Lk - 1;  // masked later
      regK[i] = *reinterpret_cast<const f16x8*>(&kb[(long)krow * k_row + st_c8[i]]);
      regV[i] = *reinterpret_cast<const f16x8*>(&vb[(long)krow * k_row + st_c8[i]]);
    }
  };

  stage_load(0);
  for (int t0 = 0; t0 < Lk; t0 += KT) {
    if (t0) __syncthreads();  // previous tile's reads complete
#pragma unroll
    for (int i = 0; i < LOADS_PT; ++i) {
      if (st_row[i] >= KT) continue;
      *reinterpret_cast<f16x8*>(&ldsK[st_row[i] * KPITCH + st_c8[i]]) = regK[i];
      *reinterpret_cast<f16x8*>(&ldsV[st_row[i] * KPITCH + st_c8[i]]) = regV[i];
    }
    __syncthreads();
    if (t0 + KT < Lk) stage_load(t0 + KT);

    // ---- S = scale * Q K^T  (QF x NF col fragments of 16) ----
    f32x4 sfrag[QF][NF];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const f16* kr = &ldsK[(nf * 16 + (lane & 15)) * KPITCH + fcol];
#pragma unroll
      for (int ds = 0; ds < D32; ++ds) {
        f16x8 bfrag = *reinterpret_cast<const f16x8*>(kr + ds * 32);
#pragma unroll
        for (int qi = 0; qi < QF; ++qi) {
          if (ds == 0) sfrag[qi][nf] = {0.f, 0.f, 0.f, 0.f};
          sfrag[qi][nf] = mfma16x16x32(aq[qi][ds], bfrag, sfrag[qi][nf]);
        }
      }
    }

    // ---- online softmax update (rows lane-local), per q-fragment ----
#pragma unroll
    for (int qi = 0; qi < QF; ++qi) {
      float p[NF][4];  // [nf][reg j]
      float mnew[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) mnew[j] = -1e30f;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        const int kcol = t0 + nf * 16 + (lane & 15);
        const bool valid = kcol < Lk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float val = valid ? sfrag[qi][nf][j] * scale2 : -1e30f;
          p[nf][j] = val;
          mnew[j] = fmaxf(mnew[j], val);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // 16-lane row reductions on the VALU pipe (DPP) — __shfl_xor's
        // ds_bpermute contends with this kernel's heavy LDS traffic
        // (measured: 608 bpermutes/iteration before)
        mnew[j] = quarter_reduce(mnew[j], MaxOp());
        const float mn = fmaxf(m_i[qi][j], mnew[j]);
        const float alpha = __builtin_amdgcn_exp2f(m_i[qi][j] - mn);
        float rs = 0.f;
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
          p[nf][j] = __builtin_amdgcn_exp2f(p[nf][j] - mn);
          rs += p[nf][j];
        }
        rs = quarter_reduce(rs, SumOp());
        l_i[qi][j] = l_i[qi][j] * alpha + rs;
        m_i[qi][j] = mn;
#pragma unroll
        for (int f = 0; f < D16; ++f) o_acc[qi][f][j] *= alpha;
      }

      // ---- P -> LDS transposed [kv][q] (C-frag -> A-frag bridge): the 4
      // j-values are consecutive q rows of kv column nf*16+(lane&15) ----
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        f16x4 pv;
#pragma unroll
        for (int j = 0; j < 4; ++j) pv[j] = (f16)p[nf][j];
        *reinterpret_cast<f16x4*>(
            &myP[(nf * 16 + (lane & 15)) * PT_PITCH + qi * 16 +
                 (lane >> 4) * 4]) = pv;
      }
    }
    // same-wave LDS write->read: wait for the writes, keep reads below
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- O += P V  (BOTH operands via hardware transpose reads: V from
    // its row-major tile, P from the transposed bridge tile) ----
#pragma unroll
    for (int ks = 0; ks < KT / 32; ++ks) {
      f16x8 afrag[QF];
#pragma unroll
      for (int qi = 0; qi < QF; ++qi)
        afrag[qi] = tr_bfrag(myP, PT_PITCH, ks * 32, qi * 16, lane);
#pragma unroll
      for (int f = 0; f < D16; ++f) {
        f16x8 bfrag = tr_bfrag(ldsV, KPITCH, ks * 32, f * 16, lane);
#pragma unroll
        for (int qi = 0; qi < QF; ++qi)
          o_acc[qi][f] = mfma16x16x32(afrag[qi], bfrag, o_acc[qi][f]);
      }
    }
  }

  // ---- epilogue: O /= l, masked stores ----
#pragma unroll
  for (int qi = 0; qi < QF; ++qi)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int qrow = q0 + (wid * QF + qi) * 16 + (lane >> 4) * 4 + j;
      if (qrow >= Lq) continue;
      const float inv_l = 1.0f / l_i[qi][j];
#pragma unroll
      for (int f = 0; f < D16; ++f)
        ob[(long)qrow * o_row + f * 16 + (lane & 15)] =
            (f16)(o_acc[qi][f][j] * inv_l);
    }
}

extern "C" void airtc_attention(const uint16_t* q, const uint16_t* k,
                                const uint16_t* v, uint16_t* out, int B, int H,
                                int Lq, int Lk, int d, long q_sb, long q_sh,
                                long q_row, long k_sb, long k_sh, long k_row,
                                long o_sb, long o_sh, long o_row, float scale,
                                hipStream_t s) {
  // KVT=128 tiles: half the barriers and m/l bookkeeping per key. Measured
  // (same-box A/B): L4096 B=1 115->92.5us (+25%), B=8 479->454us (+5.5%);
  // L1024 +24%/+4%; L256 B=8 regresses 7% (occupancy cliff bites when the
  // grid is small-per-key-work). DEFAULT: auto = 128 for Lk >= 1024, 64
  // below; AIRTC_ATTN_KVT=64|128 forces.
  static int kvt_env = -1;
  if (kvt_env < 0) {
    const char* e = getenv("AIRTC_ATTN_KVT");
    kvt_env = e ? atoi(e) : 0;  // 0 = auto
  }
  const int kvt_sel = kvt_env ? kvt_env : (Lk >= 1024 ? 128 : 64);
  dim3 grid(ceil_div(Lq, QT), B * H);
  const f16* qp = reinterpret_cast<const f16*>(q);
  const f16* kp = reinterpret_cast<const f16*>(k);
  const f16* vp = reinterpret_cast<const f16*>(v);
  f16* op = reinterpret_cast<f16*>(out);
#define LAUNCH_T(D, KT)                                                     \
  hipLaunchKernelGGL((attention_kernel<D, KT>), grid, dim3(256), 0, s, qp,  \
                     kp, vp, op, H, Lq, Lk, q_sb, q_sh, q_row, k_sb, k_sh,  \
                     k_row, o_sb, o_sh, o_row, scale)
#define LAUNCH(D)                                                           \
  do {                                                                      \
    if (kvt_sel == 128 && Lk >= 128) LAUNCH_T(D, 128);                      \
    else LAUNCH_T(D, 64);                                                   \
  } while (0)
  switch (d) {
    case 32: LAUNCH(32); break;
    case 64: LAUNCH(64); break;
    case 96: LAUNCH(96); break;
    case 128: LAUNCH(128); break;
    case 160: LAUNCH(160); break;
    default: break;  // host wrapper guarantees one of the above
  }
#undef LAUNCH
#undef LAUNCH_T
}
