// Host-visible launcher declarations for the MI355X kernels.
// Interfaces use uint16_t* for f16 storage so the host translation unit
// (compiled by g++) never needs _Float16.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

// elementwise ---------------------------------------------------------------
void airtc_preprocess_u8(const uint8_t* in, uint16_t* out, long n, hipStream_t s);
void airtc_postprocess_u8(const uint16_t* in, uint8_t* out, long n, hipStream_t s);
void airtc_silu_f16(const uint16_t* in, uint16_t* out, long n, hipStream_t s);
void airtc_geglu_f16(const uint16_t* in, uint16_t* out, long rows, long inner,
                     hipStream_t s);
void airtc_add_act_f16(const uint16_t* a, const uint16_t* b, uint16_t* out,
                       long n, int act, hipStream_t s);
void airtc_upsample2x_f16(const uint16_t* in, uint16_t* out, int B, int H,
                          int W, int C, hipStream_t s);
// any-resolution ingest: crop src window (y0,x0,ch,cw) of a u8 RGB (Hs,Ws,3)
// frame, antialiased-triangle resize into window (oy,ox,oh,ow) of ONE
// (H,W,3) u8 slot `dst`, zeros elsewhere in the slot. Windows are validated
// by the caller (ext.cpp).
void airtc_fit_resize_u8(const uint8_t* src, int Ws, uint8_t* dst, int H,
                         int W, int y0, int x0, int ch, int cw, int oy,
                         int ox, int oh, int ow, hipStream_t s);
// same resize of window (y0,x0,ch,cw) into a whole (H,W) picture, H and W
// even, written as its I420 frame (3H/2, W) in the same launch
void airtc_fit_resize_u8_i420(const uint8_t* src, int Ws, uint8_t* dst, int H,
                              int W, int y0, int x0, int ch, int cw,
                              hipStream_t s);
// colour (color.hip) --------------------------------------------------------
// I420 frame = (3H/2, W) u8: H*W of Y, then (H/2)*(W/2) of Cb, then of Cr,
// tight; BT.601 limited range in the software codec's integer arithmetic.
// H and W even and >= 2 (validated by the caller, ext.cpp); batches are B
// tight frames.
// (B,H,W,3) u8 RGB -> (B,3H/2,W) I420
void airtc_rgb_u8_to_i420(const uint8_t* in, uint8_t* out, int B, int H,
                          int W, hipStream_t s);
// (B,H,W,3) f16 in [-1,1] -> I420: postprocess_u8 fused with the above
void airtc_postprocess_i420(const uint16_t* in, uint8_t* out, int B, int H,
                            int W, hipStream_t s);
// (B,3H/2,W) I420 -> (B,H,W,3) u8 RGB, chroma nearest-replicated
void airtc_i420_to_rgb_u8(const uint8_t* in, uint8_t* out, int B, int H,
                          int W, hipStream_t s);
// edge hint (canny.hip) -----------------------------------------------------
// (B,H,W,3) u8 RGB -> (B,H,W,3) f16 (out_f32 == 0) or f32, three equal
// channels, 1.0 on an edge: integer Canny with hysteresis bounded to `reach`
// (0..32) 3x3 steps, one launch, no scratch. thr is (B,2) i32 (low, high)
// per row, read on the device. Any H, W >= 1. Returns -1 and launches
// nothing on a reach or grid out of range.
int airtc_canny_hint(const uint8_t* in, const int* thr, void* out,
                     int out_f32, int B, int H, int W, int reach,
                     hipStream_t s);
// CLIP safety checker (safety.hip) -------------------------------------------
// (B,H,W,3) f16 decoder image -> (B, (size/patch)^2, 3*patch^2) f16 patches
// in (c, py, px) order: post_u8 per pixel, antialiased bicubic resize to
// (nh, nw), round to u8, the size x size window at (top, left), then
// lut[c*256 + v] (3x256 f16: (v/255 - mean_c)/std_c). Geometry is validated
// by the caller (ext.cpp): size % patch == 0, top + size <= nh,
// left + size <= nw, B <= 65535.
void airtc_clip_patches(const uint16_t* img, uint16_t* out,
                        const uint16_t* lut, int B, int H, int W, int size,
                        int patch, int nh, int nw, int top, int left,
                        hipStream_t s);
// x * sigmoid(1.702 x), n % 8 == 0
void airtc_quick_gelu_f16(const uint16_t* in, uint16_t* out, long n,
                          hipStream_t s);
// dynamic LDS the head kernel asks for; the caller keeps it under 64 KB
int airtc_safety_head_lds_bytes(int hidden, int proj, int ns, int nc);
// class token (B rows of `hidden` f16, cls_stride elements apart) ->
// LayerNorm (f32 g, b) -> proj_w (proj, hidden) f16 GEMV -> cosines against
// unit-norm f32 tables special (ns, proj) and concept (nc, proj) -> the
// checker's decision with adjust[b]: flags (B,) i32, scores (B, ns + nc) f32
// (special first), counters[b] += flag. hidden % 8 == 0; cls rows and proj_w
// 16-byte aligned.
void airtc_safety_head(const uint16_t* cls, long cls_stride, const float* ln_g,
                       const float* ln_b, const uint16_t* proj_w,
                       const float* special, const float* special_w,
                       const float* concept, const float* concept_w,
                       const float* adjust, int* counters, int* flags,
                       float* scores, int B, int hidden, int proj, int ns,
                       int nc, float eps, hipStream_t s);
// frames b of img (B rows of `per` f16) with flags[b] != 0 become -1, in
// place. vec != 0: per % 8 == 0 and img 16-byte aligned.
void airtc_blank_flagged(uint16_t* img, const int* flags, int B, long per,
                         int vec, hipStream_t s);
// fused LCM scheduler math (one kernel each; coefficients are per-batch-row
// f32 arrays of B entries, per_b = elements per batch row)
void airtc_sched_add_noise(const uint16_t* x0, const uint16_t* noise,
                           const float* a, const float* bt, uint16_t* out,
                           long per_b, long n, hipStream_t s);
void airtc_sched_blend(const uint16_t* xt, const uint16_t* eps,
                       const float* a, const float* bt, const float* c_out,
                       const float* c_skip, uint16_t* out, long per_b, long n,
                       hipStream_t s);
// residual-CFG step in one launch, per-row f32 coefficients of B entries
// (B = output rows). mode 0 self: eps (B), stock (B) read then shifted in
// place; 1 initialize: eps = [seed(fbs) | cond(B)]; 2 full: eps =
// [uncond(B) | cond(B)], gm1 holds g, stock/delta unused (may be null).
// vec != 0 selects the 16-byte path: per_b % 8 == 0, pointers 16-B aligned.
void airtc_rcfg_apply(int mode, const uint16_t* eps, uint16_t* stock,
                      const float* gm1, const float* delta, uint16_t* out,
                      long B, long fbs, long per_b, int vec, hipStream_t s);

// norms ---------------------------------------------------------------------
// GroupNorm partial statistics, the one layout every producer and consumer
// shares: f32 [B*G][npart][2] = per (batch, group), npart partial
// (sum, sumsq) pairs over disjoint parts of the group's HW*Cg elements;
// consumers add the npart pairs in index order. npart is chosen by the
// producer and is <= AIRTC_GN_MAX_PART, so a ws of
// B*G*AIRTC_GN_MAX_PART*2 floats always fits.
#define AIRTC_GN_MAX_PART 64
int airtc_group_norm_nchunk(int B, int G);
// GroupNorm + act. part == nullptr: the statistics pass runs first, into ws
// (B*G*AIRTC_GN_MAX_PART*2 floats). Otherwise apply only, on npart partials
// from another producer (the split-K finalize with gn_part below); ws is
// unused. Exactly one of out / out_q8 is non-null: f16 result, or e4m3
// codes q = clamp(act(gn(x)) / a_scale) (producer-side quantization for the
// fp8 conv path).
void airtc_group_norm(const uint16_t* x, const float* part, int npart,
                      const float* gamma, const float* beta, uint16_t* out,
                      uint8_t* out_q8, float* ws, int B, int HW, int C, int G,
                      float eps, int act, float a_scale, hipStream_t s);
void airtc_layer_norm(const uint16_t* x, const float* gamma, const float* beta,
                      uint16_t* out, long rows, int C, float eps,
                      hipStream_t s);
// (B, C, 2) f32 affine pairs for the fused GN->conv input transform; ws as
// above
void airtc_group_norm_coeffs(const uint16_t* x, const float* gamma,
                             const float* beta, float* coeffs, float* ws,
                             int B, int HW, int C, int G, float eps,
                             hipStream_t s);

// conv ----------------------------------------------------------------------
// One conv problem: the record every conv launcher takes. The host (ext.cpp,
// conv_problem) fills and validates it; the launchers trust it.
typedef struct AirtcConvArgs {
  // (B, H >> up, W >> up, IC) NHWC f16, zero padding handled inline; the fp8
  // launcher with x_is_q8 reads u8 e4m3 codes here instead
  const void* x;
  // the weight in the launcher's own layout: mfma / direct (OC, R*S*IC + IC2)
  // f16, k order (r, s, ic) then the x2 segment; tinyic the (36, OC) f32 pack
  // (row k = GEMM column k, rows past R*S*IC zero); fp8 (OC, R*S*IC) OCP e4m3
  // bytes, quantized per OC on the host
  const void* w;
  const float* bias;         // optional (OC,) f32
  const uint16_t* cbias;     // optional (B, OC) f16 per-(batch, out-channel)
                             // bias: the time-embedding add
  const uint16_t* residual;  // optional f16 of out's shape, added before act
  uint16_t* out;             // (B, HO, WO, OC) f16
  float* ws;                 // f32 split-K workspace (B*k, HO*WO, OC),
                             // required when path is +-k with k > 1
  // optional (B, IC, 2) f32 per-channel input affine (fused GroupNorm) with
  // in_act applied after: transforms x AT LOAD TIME, padding stays zero.
  // Applies to x only, never to x2. mfma, direct and fp8 (f16 x).
  const float* in_aff;
  // optional second K segment (mfma only): a (B, HO, WO, IC2) f16 tensor read
  // as a 1x1 stride-1 tap at the output pixel, a resnet's pointwise shortcut.
  // Needs stride == 1 and IC2 % 32 == 0; excludes up.
  const uint16_t* x2;
  // optional GroupNorm partials of the OUTPUT for a consumer norm with
  // gn_groups groups (layout above), written by the split-K finalize from
  // the rounded f16 values (mfma only). Pass it only when
  // airtc_conv2d_stats_nchunk returns npart > 0 (split-K path, act ==
  // ACT_NONE, OC % 4 == 0, even OC/G, B <= 65535); B*G*npart*2 floats; bias /
  // cbias / residual 16 B aligned.
  float* gn_part;
  int B, H, W, IC;  // H, W: the extents the conv sees (upsampled when up)
  int HO, WO, OC;
  int R, S, stride, pad;
  int pad_hi;   // extra zero rows / columns below and right of the input only
                // (HO, WO count them); the kernels' hi < H, wi < W predicates
                // already zero those taps
  int act;      // epilogue: out = act(conv + bias + cbias + residual)
  int in_act;   // with in_aff
  int path;     // airtc_conv2d_splitk_for: 0 = direct, +k = BM128 split-K k,
                // -k = BM64 split-K k (mfma, fp8: nonzero)
  int IC2;      // channels of x2, 0 without
  int up;       // 1 = x is read through nearest-2x addressing (mfma only)
  int gn_groups;  // with gn_part
} AirtcConvArgs;

int airtc_conv2d_splitk_for(int B, int HO, int WO, int OC, int IC);
// partials the split-K finalize would write for this shape (see gn_part), 0
// when it cannot produce them
int airtc_conv2d_stats_nchunk(int B, int HO, int WO, int OC, int IC, int G,
                              int act);
// implicit-GEMM MFMA conv (IC % 32 == 0). Returns 1 when gn_part was written,
// 0 otherwise (the caller must then drop the buffer: nothing initialised
// it), -1 and launches nothing when x2 and up are both set.
int airtc_conv2d_mfma(const AirtcConvArgs* a, hipStream_t s);
// ragged IC: the small-IC kernel up to K = 288, else one thread per output
void airtc_conv2d_direct(const AirtcConvArgs* a, hipStream_t s);
// tiny-IC conv (IC <= 4, R*S*IC <= 36; airtc_conv2d_tinyic_ok): lanes along OC
int airtc_conv2d_tinyic_ok(int IC, int R, int S);
void airtc_conv2d_tinyic(const AirtcConvArgs* a, hipStream_t s);

// fp8 (MX-scaled MFMA path) -------------------------------------------------
// conv2d on v_mfma_scale_f32_16x16x128_f8f6f4 (conv2d_fp8.hip). dq[oc] =
// a_scale * w_scale[oc] dequantizes in the epilogue; activations quantize in
// the staging loads (a_scale). Requires IC % 64 == 0.
// x_is_q8: x already holds e4m3 codes (u8, producer-quantized by e.g.
// airtc_group_norm with out_q8): staging is a raw byte copy, in_aff unused.
// out_q8/out_inv: when non-null and split-K == 1, the epilogue writes e4m3
// codes q = e4m3(clamp(v / out_scale)) instead of f16 (chained fp8 layers).
void airtc_conv2d_fp8_mfma(const AirtcConvArgs* a, const float* dq,
                           float a_scale, int x_is_q8, uint8_t* out_q8,
                           float out_inv, hipStream_t s);
// hardware probes: raw-fragment MX MFMA tile and the fused scale-converts
// (layout/semantics verified on hardware before the fp8 conv relies on them)
void airtc_fp8_mx_probe(const uint8_t* A, const uint8_t* B, float* draw,
                        int sa, int sb, hipStream_t s);
void airtc_fp8_cvt_probe(const uint16_t* fin, float scale, uint8_t* enc_out,
                         const uint8_t* enc_in, uint16_t* dec_out,
                         hipStream_t s);
void airtc_fp8_quant_probe(const uint16_t* in16, float sa, uint8_t* out16,
                           int variant, hipStream_t s);

// attention -----------------------------------------------------------------
// q: base+strides address (B,H) heads; row stride in elements.
// all of q/k/v/out share the (b,h) base law: base = b*sb + h*sh
void airtc_attention(const uint16_t* q, const uint16_t* k, const uint16_t* v,
                     uint16_t* out, int B, int H, int Lq, int Lk, int d,
                     long q_sb, long q_sh, long q_row, long k_sb, long k_sh,
                     long k_row, long o_sb, long o_sh, long o_row, float scale,
                     hipStream_t s);
// one wide head (attention_wide.hip): same contract, d with
// airtc_attention_wide_ok (512). 0, or < 0 when the device refused the
// kernel's dynamic LDS (nothing launched).
int airtc_attention_wide_ok(int d);
int airtc_attention_wide(const uint16_t* q, const uint16_t* k,
                         const uint16_t* v, uint16_t* out, int B, int H, int Lq,
                         int Lk, int d, long q_sb, long q_sh, long q_row,
                         long k_sb, long k_sh, long k_row, long o_sb, long o_sh,
                         long o_row, float scale, hipStream_t s);

// per-row LoRA delta (lora.hip) ---------------------------------------------
// y[b, :, col_offset : col_offset+N] += row_scale[b] * (x[b] . A[a]^T) . B[a]^T
// in place, a = row_adapter[b]; rows with a < 0 (or a >= n_adapters) are not
// read or written. x (Bt, L, K), y (Bt, L, Ny), A (n_adapters, R, K),
// B (n_adapters, N, R), f16, x / A / B 16-byte and y 8-byte aligned. Needs
// K % 32 == 0, N % 16 == 0, col_offset % 16 == 0, col_offset + N <= Ny,
// Ny % 4 == 0, R in {16, 32, 64}, Bt <= 65535; the caller (ext.cpp) also keeps
// every element count within 31 bits. Returns -1 and launches nothing
// otherwise.
int airtc_lora_delta(const uint16_t* x, uint16_t* y, const uint16_t* A,
                     const uint16_t* B, const int* row_adapter,
                     const float* row_scale, int Bt, int L, int K, int N,
                     int Ny, int R, int col_offset, int n_adapters,
                     hipStream_t s);

}  // extern "C"

// vcn ------------------------------------------------------------------------
// Probe the VCN video block's VA-API userspace (runtime dlopen). Returns
// -1 = unavailable, else bit0 = H.264 decode, bit1 = H.264 encode; buf gets
// a stage/detail summary. Implemented in vcn.cpp.
extern "C" int airtc_vcn_probe(char* buf, int buflen);

// H.264 parameter-set generation (vcn.cpp): Annex-B SPS+PPS for (w, h).
extern "C" int airtc_h264_sps_pps(int width, int height, uint8_t* buf,
                                  int buflen);
