// Torch bindings for the MI355X HIP kernels (host-side translation unit).
//
// Thin layer: validates tensors, allocates outputs through the torch caching
// allocator (hipGraph-capture safe), and calls the extern "C" launchers from
// kernels.h on the current stream. No compute logic lives here.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <algorithm>
#include <limits>

#include "kernels.h"

#define CHECK_IN(x)                                                     \
  TORCH_CHECK(x.is_cuda(), #x " must be on GPU");                       \
  TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

namespace {

hipStream_t cur_stream() {
  return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

const uint16_t* h_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const uint16_t*>(t.data_ptr<at::Half>());
}
uint16_t* h_ptr_mut(torch::Tensor& t) {
  return reinterpret_cast<uint16_t*>(t.data_ptr<at::Half>());
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

using OptTensor = c10::optional<torch::Tensor>;
constexpr int64_t kIntMax = std::numeric_limits<int>::max();
constexpr int64_t kGridYZ = 65535;  // largest gridDim.y / gridDim.z

// an operand a kernel reads: on x's device, contiguous, of dtype dt
void check_operand(const torch::Tensor& t, const torch::Tensor& x,
                   c10::ScalarType dt, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.device() == x.device(), what,
              " must be on the input's GPU");
  TORCH_CHECK(t.is_contiguous(), what, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == dt, what, " must be ", dt, ", got ",
              t.scalar_type());
}

// the same operand with its element count
void check_operand(const torch::Tensor& t, const torch::Tensor& x,
                   c10::ScalarType dt, int64_t n, const char* what) {
  check_operand(t, x, dt, what);
  TORCH_CHECK(t.numel() == n, what, " must hold ", n, " values, got ",
              t.numel());
}

// an optional one: its pointer, null when absent
template <typename T>
const T* opt_operand(const OptTensor& t, const torch::Tensor& x,
                     c10::ScalarType dt, int64_t n, const char* what) {
  if (!t.has_value()) return nullptr;
  check_operand(*t, x, dt, n, what);
  return static_cast<const T*>(t->data_ptr());
}

// --- conv (conv2d.hip, conv2d_fp8.hip) ---------------------------------
// which launcher the problem is for: it decides the weight layout, the
// input dtype and the operands that may come along
enum ConvKind { CONV_F16, CONV_TINYIC, CONV_FP8 };

struct ConvProblem {
  AirtcConvArgs a = {};
  torch::Tensor out, ws;  // own a.out and a.ws
  bool empty = false;     // no output element: nothing to launch
};

// The one place a conv's tensors become a launcher record: derives the
// extents, validates every operand, refuses sizes the kernels' index
// arithmetic cannot hold, allocates the output and the split-K workspace.
// want_q8 (fp8): u8 e4m3 output where the shape takes no split-K, since the
// finalize pass stays fp8-agnostic; callers dispatch on the returned dtype.
ConvProblem conv_problem(ConvKind kind, const torch::Tensor& x,
                         const torch::Tensor& w, const OptTensor& bias,
                         const OptTensor& cbias, const OptTensor& residual,
                         int64_t R, int64_t S, int64_t stride, int64_t pad,
                         int64_t pad_hi, int64_t act,
                         const OptTensor& in_affine, int64_t in_act,
                         const OptTensor& x2, bool upsample2x, bool want_q8) {
  ConvProblem p;
  AirtcConvArgs& a = p.a;
  const bool x_q8 = kind == CONV_FP8 && x.scalar_type() == torch::kByte;
  check_operand(x, x, x_q8 ? torch::kByte : torch::kHalf, "x");
  check_operand(w, x,
                kind == CONV_F16      ? torch::kHalf
                : kind == CONV_TINYIC ? torch::kFloat
                                      : torch::kByte,
                "w");
  TORCH_CHECK(x.dim() == 4 && w.dim() == 2,
              "x must be (B, H, W, IC) and the weight 2-D");
  TORCH_CHECK(R >= 1 && S >= 1 && stride >= 1 && pad >= 0, "conv needs R, S ",
              ">= 1, stride >= 1, pad >= 0, got ", R, "x", S, " stride ",
              stride, " pad ", pad);
  // pad_hi: extra zero rows / columns at the bottom / right only
  TORCH_CHECK(pad_hi >= 0, "conv needs pad_hi >= 0, got ", pad_hi);
  TORCH_CHECK(kind != CONV_FP8 || pad_hi == 0,
              "the fp8 conv takes no bottom/right-only padding");
  const int up = upsample2x ? 1 : 0;
  const int64_t B = x.size(0), IC = x.size(3);
  const int64_t H = x.size(1) << up, W = x.size(2) << up;
  const int64_t OC = kind == CONV_TINYIC ? w.size(1) : w.size(0);
  // every extent is an int in the kernels, and so is a tap's coordinate
  // hi = ho * stride + r - pad < H + pad + pad_hi (the last tap of the last
  // output row ends the padded input): 2^29 each keeps both in range
  TORCH_CHECK(std::max({B, H, W, IC, OC, R, S, stride, pad, pad_hi}) <=
                  (1 << 29),
              "conv extents must stay within 2^29");
  TORCH_CHECK(IC >= 1, "conv needs input channels");
  // (C++ division truncates towards zero, so test before dividing)
  const int64_t HP = H + 2 * pad + pad_hi, WP = W + 2 * pad + pad_hi;
  TORCH_CHECK(HP >= R && WP >= S, "kernel ", R, "x", S,
              " is larger than the padded input ", HP, "x", WP);
  const int64_t HO = (HP - R) / stride + 1;
  const int64_t WO = (WP - S) / stride + 1;
  const int64_t M = HO * WO;
  // M = HO * WO is an int in every kernel
  TORCH_CHECK(M <= kIntMax, "HO * WO must fit 31 bits");

  int64_t IC2 = 0;
  if (x2.has_value()) {
    check_operand(*x2, x, torch::kHalf, "x2");
    TORCH_CHECK(x2->dim() == 4 && x2->size(0) == B && x2->size(1) == HO &&
                    x2->size(2) == WO,
                "x2 must be (B, HO, WO, IC2)");
    IC2 = x2->size(3);
    TORCH_CHECK(stride == 1 && IC2 > 0 && IC2 % 32 == 0,
                "x2 needs stride 1 and IC2 % 32 == 0");
    // the kernel offsets x2 per batch in 32 bits:
    // (ho * WO + wo) * IC2 + k8 in load_tile
    TORCH_CHECK(M * IC2 < (1L << 31), "x2 too large");
    a.x2 = h_ptr(*x2);
  }
  TORCH_CHECK(!(a.x2 && up), "x2 and upsample2x exclude each other");
  // K = R*S*IC + IC2 is an int, and the fp8 K loop forms kt * 128 + 64
  // one tile past it
  TORCH_CHECK(R * S <= kIntMax && R * S * IC + IC2 <= kIntMax - 192,
              "R * S * IC + IC2 must fit 31 bits");
  const int64_t K = R * S * IC + IC2;
  if (kind == CONV_TINYIC) {
    TORCH_CHECK(airtc_conv2d_tinyic_ok((int)IC, (int)R, (int)S),
                "conv2d_tinyic needs IC <= 4 and R*S*IC <= 36");
    TORCH_CHECK(w.size(0) == 36, "w_tiny must be (36, OC) f32");
  } else {
    TORCH_CHECK(w.size(1) == K, "the weight must be (OC, R*S*IC + IC2) = (",
                OC, ", ", K, "), got (", w.size(0), ", ", w.size(1), ")");
    TORCH_CHECK(kind != CONV_FP8 || IC % 64 == 0,
                "fp8 conv path requires IC % 64 == 0");
  }

  // 0 = direct, +k = BM128 split-K k, -k = BM64 split-K k; the fp8 kernel
  // has no direct form and picks a geometry by M
  p.empty = B == 0 || OC == 0;
  int path = 0;
  if (!p.empty && kind != CONV_TINYIC) {
    path = airtc_conv2d_splitk_for((int)B, (int)HO, (int)WO, (int)OC, (int)IC);
    if (kind == CONV_FP8 && path == 0) path = M >= 2048 ? 1 : -1;
  }
  const int64_t splitk = path > 0 ? path : -path;
  TORCH_CHECK(kind == CONV_F16 || (!a.x2 && !up),
              "x2 / upsample2x belong to the f16 MFMA conv");
  TORCH_CHECK(p.empty || path != 0 || (!a.x2 && !up),
              "x2 / upsample2x need the MFMA path (IC % 32 == 0)");
  const bool q8 = want_q8 && splitk == 1;
  p.out = torch::empty({B, HO, WO, OC},
                       x.options().dtype(q8 ? torch::kByte : torch::kHalf));

  a.bias = opt_operand<float>(bias, x, torch::kFloat, OC, "bias");
  a.cbias = opt_operand<uint16_t>(cbias, x, torch::kHalf, B * OC, "cbias");
  a.residual = opt_operand<uint16_t>(residual, x, torch::kHalf, p.out.numel(),
                                     "residual");
  a.in_aff = opt_operand<float>(in_affine, x, torch::kFloat, B * IC * 2,
                                "in_affine (B, IC, 2)");
  TORCH_CHECK(!a.in_aff || (kind != CONV_TINYIC && !x_q8),
              "the tiny-IC kernel and pre-quantized input take no fused "
              "input affine");
  if (p.empty) return p;

  if (kind == CONV_TINYIC) {
    // grid = (ceil(B*M / ppb), ceil(OC / 64)) with ppb >= 8
    TORCH_CHECK((B * M + 7) / 8 <= kIntMax && OC <= kGridYZ * 64,
                "conv2d_tinyic: too many pixels or channels for one grid");
  } else if (path == 0) {
    // small-IC kernel: grid.y = ceil(OC / 64); its grid.x and the direct
    // kernel's grid are capped and stride in 64 bits
    TORCH_CHECK(OC <= kGridYZ * 64, "conv2d: too many output channels");
  } else {
    // grid = (ceil(M / BM) * ceil(OC / 64), 1, B * splitk)
    const int64_t bm = path > 0 ? 128 : 64;
    TORCH_CHECK(B * splitk <= kGridYZ, "conv2d: batch ", B, " x split-K ",
                splitk, " exceeds the grid's z extent");
    TORCH_CHECK((M + bm - 1) / bm * ((OC + 63) / 64) <= kIntMax,
                "conv2d: too many tiles for one grid");
    // the vectorized finalize puts OC / (4 * ct) <= OC / 4 tiles in grid.y
    TORCH_CHECK(splitk == 1 || OC <= kGridYZ * 4,
                "conv2d: too many output channels for the split-K finalize");
  }
  if (splitk > 1) {
    p.ws = torch::empty({B * splitk, M, OC}, x.options().dtype(torch::kFloat));
    a.ws = p.ws.data_ptr<float>();
  }
  a.x = x.data_ptr();
  a.w = w.data_ptr();
  a.out = q8 ? nullptr : h_ptr_mut(p.out);
  a.B = B, a.H = H, a.W = W, a.IC = IC, a.HO = HO, a.WO = WO, a.OC = OC;
  a.R = R, a.S = S, a.stride = stride, a.pad = pad, a.pad_hi = pad_hi;
  a.act = act, a.in_act = in_act, a.path = path, a.IC2 = IC2, a.up = up;
  return p;
}

// f16 conv. stats_groups > 0 asks the split-K finalize for GroupNorm
// partials of the output (kernels.h layout) for a consumer norm with that
// many groups: (out, partials), or (out, None) when the shape takes no
// finalize pass or the finalize cannot produce them.
// x2: optional second K segment (B, HO, WO, IC2), w_perm then (OC, R*S*IC +
// IC2); upsample2x: x is read through nearest-2x addressing (MFMA path only)
pybind11::tuple conv2d(torch::Tensor x, torch::Tensor w_perm, OptTensor bias,
                       OptTensor cbias, OptTensor residual, int64_t R,
                       int64_t S, int64_t stride, int64_t pad, int64_t act,
                       OptTensor in_affine, int64_t in_act,
                       int64_t stats_groups, OptTensor x2, bool upsample2x,
                       int64_t pad_hi) {
  TORCH_CHECK(stats_groups >= 0 && stats_groups <= kIntMax,
              "stats_groups out of range");
  auto p = conv_problem(CONV_F16, x, w_perm, bias, cbias, residual, R, S,
                        stride, pad, pad_hi, act, in_affine, in_act, x2,
                        upsample2x, false);
  AirtcConvArgs& a = p.a;
  torch::Tensor part;
  if (p.empty) return pybind11::make_tuple(p.out, pybind11::none());
  if (a.path == 0) {
    airtc_conv2d_direct(&a, cur_stream());
  } else {
    a.gn_groups = (int)stats_groups;
    if (stats_groups > 0 && aligned16(a.bias) && aligned16(a.cbias) &&
        aligned16(a.residual)) {
      const int npart = airtc_conv2d_stats_nchunk(a.B, a.HO, a.WO, a.OC, a.IC,
                                                  a.gn_groups, a.act);
      if (npart > 0) {
        part = torch::empty({a.B * stats_groups, npart, 2},
                            x.options().dtype(torch::kFloat));
        a.gn_part = part.data_ptr<float>();
      }
    }
    // the launcher has the last word: partials it did not write are dropped,
    // and the consumer norm runs its own statistics pass
    if (!airtc_conv2d_mfma(&a, cur_stream())) part = torch::Tensor();
  }
  if (part.defined()) return pybind11::make_tuple(p.out, part);
  return pybind11::make_tuple(p.out, pybind11::none());
}

// tiny-IC conv (IC <= 4, K <= 36): lanes along OC (conv2d.hip). w_tiny is the
// (36, OC) f32 pack of the weight.
torch::Tensor conv2d_tinyic(torch::Tensor x, torch::Tensor w_tiny,
                            OptTensor bias, OptTensor cbias,
                            OptTensor residual, int64_t R, int64_t S,
                            int64_t stride, int64_t pad, int64_t act,
                            int64_t pad_hi) {
  auto p = conv_problem(CONV_TINYIC, x, w_tiny, bias, cbias, residual, R, S,
                        stride, pad, pad_hi, act, c10::nullopt, 0,
                        c10::nullopt, false, false);
  if (!p.empty) airtc_conv2d_tinyic(&p.a, cur_stream());
  return p.out;
}

// fp8 conv: MX-scaled MFMA path (conv2d_fp8.hip). Same surface as conv2d
// but weights are pre-quantized e4m3 bytes + per-OC dequant scales, and the
// activation scale rides along as a scalar. out_scale > 0 asks for e4m3
// output (conv_problem, want_q8).
torch::Tensor conv2d_fp8(torch::Tensor x, torch::Tensor w_fp8,
                         torch::Tensor dq, double a_scale, OptTensor bias,
                         OptTensor cbias, OptTensor residual, int64_t R,
                         int64_t S, int64_t stride, int64_t pad, int64_t act,
                         OptTensor in_affine, int64_t in_act,
                         double out_scale) {
  auto p = conv_problem(CONV_FP8, x, w_fp8, bias, cbias, residual, R, S,
                        stride, pad, 0, act, in_affine, in_act, c10::nullopt,
                        false, out_scale > 0);
  check_operand(dq, x, torch::kFloat, w_fp8.size(0), "dq (f32[OC])");
  if (p.empty) return p.out;
  const bool q8 = p.out.scalar_type() == torch::kByte;
  airtc_conv2d_fp8_mfma(&p.a, dq.data_ptr<float>(), (float)a_scale,
                        x.scalar_type() == torch::kByte ? 1 : 0,
                        q8 ? p.out.data_ptr<uint8_t>() : nullptr,
                        q8 ? (float)(1.0 / out_scale) : 0.f, cur_stream());
  return p.out;
}

// --- GroupNorm (norms.hip) ---------------------------------------------
// the operands every GroupNorm binding shares; x is (B, ..., C)
struct GnShape {
  int B, HW, C;
};

GnShape check_group_norm(const torch::Tensor& x, int64_t groups,
                         const torch::Tensor& gamma,
                         const torch::Tensor& beta) {
  check_operand(x, x, torch::kHalf, "x");
  TORCH_CHECK(x.dim() >= 2, "group_norm: x must be (B, ..., C)");
  const int64_t B = x.size(0), C = x.size(-1);
  // the kernels read channel pairs that must not straddle a group
  TORCH_CHECK(groups >= 1 && C % groups == 0 && (C / groups) % 2 == 0,
              "group_norm: groups must divide C into an even number of "
              "channels each, got C=", C, " groups=", groups);
  check_operand(gamma, x, torch::kFloat, C, "gamma");
  check_operand(beta, x, torch::kFloat, C, "beta");
  const int64_t HW = B * C > 0 ? x.numel() / (B * C) : 0;
  // grid.x = B * G blocks (airtc_group_norm_nchunk forms B * G in an int as
  // well), and HW and C are ints in the kernels; the workspace of
  // B * G * AIRTC_GN_MAX_PART pairs is then addressed in 64 bits
  TORCH_CHECK(B * groups <= kIntMax && HW <= kIntMax && C <= kIntMax,
              "group_norm: B*G, HW and C must fit 31 bits");
  return {(int)B, (int)HW, (int)C};
}

torch::Tensor gn_workspace(const torch::Tensor& x, int B, int64_t groups) {
  return torch::empty({B * groups * AIRTC_GN_MAX_PART * 2},
                      x.options().dtype(torch::kFloat));
}

torch::Tensor group_norm_coeffs(torch::Tensor x, int64_t groups,
                                torch::Tensor gamma, torch::Tensor beta,
                                double eps) {
  const GnShape d = check_group_norm(x, groups, gamma, beta);
  auto coeffs = torch::empty({d.B, d.C, 2}, x.options().dtype(torch::kFloat));
  if (coeffs.numel() == 0) return coeffs;
  auto ws = gn_workspace(x, d.B, groups);
  airtc_group_norm_coeffs(h_ptr(x), gamma.data_ptr<float>(),
                          beta.data_ptr<float>(), coeffs.data_ptr<float>(),
                          ws.data_ptr<float>(), d.B, d.HW, d.C, (int)groups,
                          (float)eps, cur_stream());
  return coeffs;
}

// partials handed over by a producer (conv2d_stats): validated here, the
// launcher trusts the count
int check_partials(const torch::Tensor& p, int B, int64_t groups) {
  CHECK_IN(p);
  TORCH_CHECK(p.dtype() == torch::kFloat && p.dim() == 3 &&
                  p.size(0) == (long)B * groups && p.size(2) == 2 &&
                  p.size(1) >= 1 && p.size(1) <= AIRTC_GN_MAX_PART,
              "partials must be f32 (B*G, npart <= 64, 2)");
  return (int)p.size(1);
}

// GroupNorm + act into out (f16, or u8 e4m3 codes at a_scale): on the
// producer's partials when given, else after an own statistics pass
torch::Tensor group_norm_into(const torch::Tensor& x, torch::Tensor out,
                              int64_t groups, const torch::Tensor& gamma,
                              const torch::Tensor& beta, double eps,
                              int64_t act, double a_scale,
                              const c10::optional<torch::Tensor>& partials) {
  const GnShape d = check_group_norm(x, groups, gamma, beta);
  if (x.numel() == 0) return out;
  const bool q8 = out.dtype() == torch::kUInt8;
  const float* part = nullptr;
  int npart = 0;
  torch::Tensor ws;
  float* wsp = nullptr;
  if (partials.has_value()) {
    npart = check_partials(*partials, d.B, groups);
    part = partials->data_ptr<float>();
  } else {
    ws = gn_workspace(x, d.B, groups);
    wsp = ws.data_ptr<float>();
  }
  airtc_group_norm(h_ptr(x), part, npart, gamma.data_ptr<float>(),
                   beta.data_ptr<float>(), q8 ? nullptr : h_ptr_mut(out),
                   q8 ? out.data_ptr<uint8_t>() : nullptr, wsp, d.B, d.HW, d.C,
                   (int)groups, (float)eps, (int)act, (float)a_scale,
                   cur_stream());
  return out;
}

torch::Tensor group_norm_silu_fp8(torch::Tensor x, int64_t groups,
                                  torch::Tensor gamma, torch::Tensor beta,
                                  double eps, int64_t act, double a_scale,
                                  c10::optional<torch::Tensor> partials) {
  auto out = torch::empty_like(x, x.options().dtype(torch::kUInt8));
  return group_norm_into(x, out, groups, gamma, beta, eps, act, a_scale,
                         partials);
}

torch::Tensor group_norm_silu(torch::Tensor x, int64_t groups,
                              torch::Tensor gamma, torch::Tensor beta,
                              double eps, int64_t act,
                              c10::optional<torch::Tensor> partials) {
  return group_norm_into(x, torch::empty_like(x), groups, gamma, beta, eps,
                         act, 1.0, partials);
}

torch::Tensor layer_norm(torch::Tensor x, torch::Tensor gamma,
                         torch::Tensor beta, double eps) {
  CHECK_IN(x);
  TORCH_CHECK(x.dtype() == torch::kHalf, "layer_norm: x must be float16");
  const int C = x.size(-1);
  TORCH_CHECK(C > 0 && C % 8 == 0,
              "layer_norm: the kernel reads 8 channels per lane, C = ", C);
  TORCH_CHECK(gamma.numel() == C && beta.numel() == C,
              "layer_norm: gamma/beta must hold C values");
  const long rows = x.numel() / C;
  auto out = torch::empty_like(x);
  if (rows == 0) return out;
  airtc_layer_norm(h_ptr(x), gamma.data_ptr<float>(), beta.data_ptr<float>(),
                   h_ptr_mut(out), rows, C, (float)eps, cur_stream());
  return out;
}

torch::Tensor attention_bhlc(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                             int64_t heads, double scale) {
  // q/k/v: (B, L, C) with unit channel stride; row/batch strides are free so
  // chunk() views of a fused QKV projection run zero-copy.
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda(), "q/k/v must be on GPU");
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3, "q/k/v: (B, L, C)");
  TORCH_CHECK(q.dtype() == torch::kHalf && k.dtype() == torch::kHalf &&
                  v.dtype() == torch::kHalf, "q/k/v must be float16");
  TORCH_CHECK(q.stride(2) == 1, "q: unit channel stride");
  TORCH_CHECK(k.stride(2) == 1 && v.stride(2) == 1, "k/v: unit channel stride");
  TORCH_CHECK(k.sizes() == v.sizes() && k.strides() == v.strides(),
              "k/v must share layout");
  const int B = q.size(0), Lq = q.size(1), C = q.size(2);
  const int Lk = k.size(1), Ck = k.size(2);
  TORCH_CHECK(heads > 0 && C % heads == 0, "channels must split into heads");
  const int d = C / (int)heads;
  TORCH_CHECK(Ck == C && k.size(0) == B, "q/k batch or channel mismatch");
  const bool wide = airtc_attention_wide_ok(d) != 0;
  TORCH_CHECK(d > 0 && d % 32 == 0 && (d <= 160 || wide),
              "head_dim must be padded to one of 32/64/96/128/160, or be 512 "
              "(one wide head), got ", d);
  TORCH_CHECK(Lq > 0 && Lk > 0 && B > 0, "attention needs non-empty q and k");
  // the kernel reads rows with 16-byte loads: every row must start on one
  TORCH_CHECK(q.stride(1) % 8 == 0 && k.stride(1) % 8 == 0 &&
                  q.stride(0) % 8 == 0 && k.stride(0) % 8 == 0,
              "q/k/v row and batch strides must be multiples of 8 elements");
  TORCH_CHECK(aligned16(q.data_ptr()) && aligned16(k.data_ptr()) &&
                  aligned16(v.data_ptr()),
              "q/k/v must start on a 16-byte boundary");
  auto out = torch::empty({B, Lq, C}, q.options());
  if (wide) {
    // attention_wide.hip: grid (ceil(Lq / 16), B * heads)
    TORCH_CHECK((int64_t)B * heads <= kGridYZ,
                "attention: batch x heads exceeds the grid's y extent");
    const int rc = airtc_attention_wide(
        h_ptr(q), h_ptr(k), h_ptr(v), h_ptr_mut(out), B, (int)heads, Lq, Lk, d,
        q.stride(0), d, q.stride(1), k.stride(0), d, k.stride(1),
        (long)Lq * C, d, C, (float)scale, cur_stream());
    TORCH_CHECK(rc == 0, "attention: the wide-head kernel could not reserve "
                "its LDS (rc=", rc, ")");
    return out;
  }
  airtc_attention(h_ptr(q), h_ptr(k), h_ptr(v), h_ptr_mut(out), B, (int)heads,
                  Lq, Lk, d, q.stride(0), d, q.stride(1), k.stride(0), d,
                  k.stride(1), (long)Lq * C, d, C, (float)scale, cur_stream());
  return out;
}

torch::Tensor silu(torch::Tensor x) {
  CHECK_IN(x);
  TORCH_CHECK(x.dtype() == torch::kHalf, "silu: x must be float16");
  TORCH_CHECK(x.numel() % 8 == 0, "silu: the kernel handles 8 elements per "
              "lane, numel must be a multiple of 8, got ", x.numel());
  auto out = torch::empty_like(x);
  if (x.numel() == 0) return out;
  airtc_silu_f16(h_ptr(x), h_ptr_mut(out), x.numel(), cur_stream());
  return out;
}

torch::Tensor geglu(torch::Tensor x) {
  CHECK_IN(x);
  TORCH_CHECK(x.dtype() == torch::kHalf, "geglu: x must be float16");
  TORCH_CHECK(x.size(-1) % 16 == 0,
              "geglu: the kernel reads 8 channels per lane of each half, the "
              "last dimension must be a multiple of 16, got ", x.size(-1));
  const long inner = x.size(-1) / 2;
  const long rows = x.numel() / (2 * inner);
  auto sizes = x.sizes().vec();
  sizes.back() = inner;
  auto out = torch::empty(sizes, x.options());
  airtc_geglu_f16(h_ptr(x), h_ptr_mut(out), rows, inner, cur_stream());
  return out;
}

torch::Tensor add_act(torch::Tensor a, torch::Tensor b, int64_t act) {
  CHECK_IN(a);
  CHECK_IN(b);
  TORCH_CHECK(a.dtype() == torch::kHalf && b.dtype() == torch::kHalf,
              "add_act: a and b must be float16");
  TORCH_CHECK(a.numel() == b.numel(), "add_act: a has ", a.numel(),
              " elements, b ", b.numel());
  TORCH_CHECK(a.numel() % 8 == 0, "add_act: numel must be a multiple of 8");
  auto out = torch::empty_like(a);
  if (a.numel() == 0) return out;
  airtc_add_act_f16(h_ptr(a), h_ptr(b), h_ptr_mut(out), a.numel(), (int)act,
                    cur_stream());
  return out;
}

torch::Tensor upsample2x(torch::Tensor x) {
  CHECK_IN(x);
  TORCH_CHECK(x.dtype() == torch::kHalf, "upsample2x: x must be float16");
  TORCH_CHECK(x.dim() == 4, "upsample2x: x must be (B, H, W, C)");
  TORCH_CHECK(x.size(3) % 8 == 0, "upsample2x: the kernel copies 8 channels "
              "per lane, C must be a multiple of 8, got ", x.size(3));
  // B, 2 * H, 2 * W and C / 8 are ints in the kernel
  TORCH_CHECK(std::max({x.size(0), x.size(1), x.size(2), x.size(3)}) <=
                  kIntMax / 2,
              "upsample2x: extents must fit 30 bits");
  const int B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  auto out = torch::empty({B, 2 * H, 2 * W, C}, x.options());
  if (out.numel() == 0) return out;
  airtc_upsample2x_f16(h_ptr(x), h_ptr_mut(out), B, H, W, C, cur_stream());
  return out;
}

torch::Tensor preprocess_u8(torch::Tensor frame) {
  CHECK_IN(frame);
  TORCH_CHECK(frame.dtype() == torch::kUInt8,
              "preprocess_u8: frame must be uint8");  // any element count
  auto out = torch::empty(frame.sizes(),
                          frame.options().dtype(torch::kHalf));
  if (frame.numel() == 0) return out;
  airtc_preprocess_u8(frame.data_ptr<uint8_t>(),
                      reinterpret_cast<uint16_t*>(out.data_ptr<at::Half>()),
                      frame.numel(), cur_stream());
  return out;
}

torch::Tensor postprocess_u8(torch::Tensor img) {
  CHECK_IN(img);
  TORCH_CHECK(img.dtype() == torch::kHalf,
              "postprocess_u8: img must be float16");  // any element count
  auto out = torch::empty(img.sizes(), img.options().dtype(torch::kUInt8));
  if (img.numel() == 0) return out;
  airtc_postprocess_u8(h_ptr(img), out.data_ptr<uint8_t>(), img.numel(),
                       cur_stream());
  return out;
}

void fit_resize_u8(torch::Tensor src, torch::Tensor dst, int64_t slot,
                   int64_t y0, int64_t x0, int64_t ch, int64_t cw, int64_t oy,
                   int64_t ox, int64_t oh, int64_t ow) {
  CHECK_IN(src);
  CHECK_IN(dst);
  TORCH_CHECK(src.dtype() == torch::kUInt8 && dst.dtype() == torch::kUInt8);
  TORCH_CHECK(src.device() == dst.device(), "src/dst on different devices");
  TORCH_CHECK(src.dim() == 3 && src.size(2) == 3, "src must be (Hs, Ws, 3)");
  TORCH_CHECK(dst.dim() == 4 && dst.size(3) == 3, "dst must be (B, H, W, 3)");
  const int64_t Hs = src.size(0), Ws = src.size(1);
  const int64_t B = dst.size(0), H = dst.size(1), W = dst.size(2);
  TORCH_CHECK(Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "empty frame");
  TORCH_CHECK(Hs * Ws * 3 < (1LL << 31) && H * W * 3 < (1LL << 31),
              "frame too large");
  TORCH_CHECK(slot >= 0 && slot < B, "slot out of range");
  // the kernel trusts these windows for every load and store
  TORCH_CHECK(ch >= 1 && cw >= 1 && y0 >= 0 && x0 >= 0 && y0 + ch <= Hs &&
                  x0 + cw <= Ws,
              "source window out of range");
  TORCH_CHECK(oh >= 1 && ow >= 1 && oy >= 0 && ox >= 0 && oy + oh <= H &&
                  ox + ow <= W,
              "destination window out of range");
  airtc_fit_resize_u8(src.data_ptr<uint8_t>(), (int)Ws,
                      dst.data_ptr<uint8_t>() + slot * H * W * 3, (int)H,
                      (int)W, (int)y0, (int)x0, (int)ch, (int)cw, (int)oy,
                      (int)ox, (int)oh, (int)ow, cur_stream());
}

// egress: window (y0,x0,ch,cw) of src (Hs,Ws,3) -> dst, a whole I420 frame
// (3H/2, W); the target size is dst's
void fit_resize_u8_i420(torch::Tensor src, torch::Tensor dst, int64_t y0,
                        int64_t x0, int64_t ch, int64_t cw) {
  CHECK_IN(src);
  CHECK_IN(dst);
  TORCH_CHECK(src.dtype() == torch::kUInt8 && dst.dtype() == torch::kUInt8);
  TORCH_CHECK(src.device() == dst.device(), "src/dst on different devices");
  TORCH_CHECK(src.dim() == 3 && src.size(2) == 3, "src must be (Hs, Ws, 3)");
  TORCH_CHECK(dst.dim() == 2, "dst must be (3H/2, W)");
  const int64_t Hs = src.size(0), Ws = src.size(1);
  const int64_t R = dst.size(0), W = dst.size(1);
  TORCH_CHECK(R >= 3 && R % 3 == 0 && W >= 2 && W % 2 == 0,
              "I420 needs (3H/2, W) with even H, W >= 2, got ", R, "x", W);
  const int64_t H = R / 3 * 2;
  TORCH_CHECK(Hs >= 1 && Ws >= 1, "empty frame");
  TORCH_CHECK(Hs * Ws * 3 < (1LL << 31) && H * W * 3 < (1LL << 31),
              "frame too large");
  // the kernel trusts this window for every load
  TORCH_CHECK(ch >= 1 && cw >= 1 && y0 >= 0 && x0 >= 0 && y0 + ch <= Hs &&
                  x0 + cw <= Ws,
              "source window out of range");
  airtc_fit_resize_u8_i420(src.data_ptr<uint8_t>(), (int)Ws,
                           dst.data_ptr<uint8_t>(), (int)H, (int)W, (int)y0,
                           (int)x0, (int)ch, (int)cw, cur_stream());
}

// --- I420 colour conversion (color.hip) --------------------------------
// shared validation: packed side `rgb` (B,H,W,3) of dtype rgb_dt, planar
// side (B,3H/2,W) u8; `out` is the caller's tensor or a fresh one
void check_rgb_side(const torch::Tensor& rgb, c10::ScalarType rgb_dt,
                    const char* what) {
  TORCH_CHECK(rgb.dtype() == rgb_dt, what, ": wrong dtype");
  TORCH_CHECK(rgb.dim() == 4 && rgb.size(3) == 3, what,
              " must be (B, H, W, 3)");
  const int64_t B = rgb.size(0), H = rgb.size(1), W = rgb.size(2);
  TORCH_CHECK(B >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0,
              "I420 needs even H, W >= 2, got ", H, "x", W);
  TORCH_CHECK(H * W * 3 < (1LL << 31) && B < (1LL << 31), "frame too large");
}

torch::Tensor i420_out(const torch::Tensor& like,
                       const c10::optional<torch::Tensor>& out,
                       at::IntArrayRef sizes) {
  if (!out.has_value())
    return torch::empty(sizes, like.options().dtype(torch::kUInt8));
  CHECK_IN((*out));
  TORCH_CHECK(out->dtype() == torch::kUInt8, "out must be uint8");
  TORCH_CHECK(out->device() == like.device(), "out on a different device");
  TORCH_CHECK(out->sizes() == sizes, "out has the wrong shape");
  return *out;
}

torch::Tensor to_i420(torch::Tensor x, c10::optional<torch::Tensor> out,
                      bool f16) {
  CHECK_IN(x);
  check_rgb_side(x, f16 ? torch::kHalf : torch::kByte, "x");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2);
  auto o = i420_out(x, out, {B, H / 2 * 3, W});
  if (f16)
    airtc_postprocess_i420(h_ptr(x), o.data_ptr<uint8_t>(), (int)B, (int)H,
                           (int)W, cur_stream());
  else
    airtc_rgb_u8_to_i420(x.data_ptr<uint8_t>(), o.data_ptr<uint8_t>(), (int)B,
                         (int)H, (int)W, cur_stream());
  return o;
}

torch::Tensor rgb_u8_to_i420(torch::Tensor x,
                             c10::optional<torch::Tensor> out) {
  return to_i420(x, out, false);
}

torch::Tensor postprocess_i420(torch::Tensor img,
                               c10::optional<torch::Tensor> out) {
  return to_i420(img, out, true);
}

torch::Tensor i420_to_rgb_u8(torch::Tensor x,
                             c10::optional<torch::Tensor> out) {
  CHECK_IN(x);
  TORCH_CHECK(x.dtype() == torch::kUInt8, "x: wrong dtype");
  TORCH_CHECK(x.dim() == 3, "x must be (B, 3H/2, W)");
  const int64_t B = x.size(0), R = x.size(1), W = x.size(2);
  TORCH_CHECK(B >= 1 && R >= 3 && R % 3 == 0 && W >= 2 && W % 2 == 0,
              "I420 needs (B, 3H/2, W) with even H, W >= 2, got ", R, "x", W);
  const int64_t H = R / 3 * 2;
  TORCH_CHECK(H * W * 3 < (1LL << 31) && B < (1LL << 31), "frame too large");
  auto o = i420_out(x, out, {B, H, W, 3});
  airtc_i420_to_rgb_u8(x.data_ptr<uint8_t>(), o.data_ptr<uint8_t>(), (int)B,
                       (int)H, (int)W, cur_stream());
  return o;
}

// --- Canny edge hint (canny.hip) ---------------------------------------
torch::Tensor canny_hint(torch::Tensor frames, torch::Tensor thr,
                         int64_t reach, torch::Tensor out) {
  CHECK_IN(frames);
  CHECK_IN(thr);
  CHECK_IN(out);
  TORCH_CHECK(frames.dtype() == torch::kUInt8, "frames must be uint8");
  TORCH_CHECK(frames.dim() == 4 && frames.size(3) == 3,
              "frames must be (B, H, W, 3)");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(B >= 1 && H >= 1 && W >= 1, "empty frame");
  TORCH_CHECK(H * W * 3 < (1LL << 31) && B < 65536, "frame too large");
  TORCH_CHECK(thr.dtype() == torch::kInt32 && thr.dim() == 2 &&
                  thr.size(0) == B && thr.size(1) == 2,
              "thr must be (B, 2) int32");
  TORCH_CHECK(reach >= 0 && reach <= 32, "reach must be in [0, 32], got ",
              reach);
  TORCH_CHECK(out.dtype() == torch::kHalf || out.dtype() == torch::kFloat,
              "out must be float16 or float32");
  TORCH_CHECK(out.sizes() == frames.sizes(), "out has the wrong shape");
  TORCH_CHECK(out.device() == frames.device() &&
                  thr.device() == frames.device(),
              "frames, thr and out must share a device");
  const int rc = airtc_canny_hint(
      frames.data_ptr<uint8_t>(), thr.data_ptr<int>(), out.data_ptr(),
      out.dtype() == torch::kFloat ? 1 : 0, (int)B, (int)H, (int)W,
      (int)reach, cur_stream());
  TORCH_CHECK(rc == 0, "canny_hint: launch refused");
  return out;
}

// --- CLIP safety checker (safety.hip) ----------------------------------
torch::Tensor clip_patches(torch::Tensor img, torch::Tensor lut, int64_t size,
                           int64_t patch, int64_t nh, int64_t nw, int64_t top,
                           int64_t left, torch::Tensor out) {
  CHECK_IN(img);
  TORCH_CHECK(img.dtype() == torch::kHalf, "clip_patches: img must be float16");
  TORCH_CHECK(img.dim() == 4 && img.size(3) == 3,
              "clip_patches: img must be (B, H, W, 3)");
  const int64_t B = img.size(0), H = img.size(1), W = img.size(2);
  TORCH_CHECK(B >= 1 && B <= kGridYZ, "clip_patches: B must be in [1, ",
              kGridYZ, "], got ", B);
  TORCH_CHECK(H >= 8 && W >= 8, "clip_patches: H and W must be >= 8, got ", H,
              "x", W);
  TORCH_CHECK(H * W * 3 <= kIntMax, "clip_patches: frame too large");
  TORCH_CHECK(patch >= 1 && size >= patch && size % patch == 0 &&
                  size * 3 <= kIntMax / 4,
              "clip_patches: size must be a multiple of patch, got ", size,
              " and ", patch);
  TORCH_CHECK(nh <= kIntMax && nw <= kIntMax && top >= 0 && left >= 0 &&
                  top + size <= nh && left + size <= nw,
              "clip_patches: the ", size, "x", size, " window at (", top, ", ",
              left, ") is not inside the resized ", nh, "x", nw);
  check_operand(lut, img, torch::kHalf, 3 * 256, "clip_patches: lut");
  const int64_t grid = size / patch;
  check_operand(out, img, torch::kHalf, B * size * size * 3,
                "clip_patches: out");
  TORCH_CHECK(out.dim() == 3 && out.size(0) == B &&
                  out.size(1) == grid * grid &&
                  out.size(2) == 3 * patch * patch,
              "clip_patches: out must be (B, ", grid * grid, ", ",
              3 * patch * patch, ")");
  airtc_clip_patches(h_ptr(img), h_ptr_mut(out), h_ptr(lut), (int)B, (int)H,
                     (int)W, (int)size, (int)patch, (int)nh, (int)nw, (int)top,
                     (int)left, cur_stream());
  return out;
}

torch::Tensor quick_gelu(torch::Tensor x) {
  CHECK_IN(x);
  TORCH_CHECK(x.dtype() == torch::kHalf, "quick_gelu: x must be float16");
  TORCH_CHECK(x.numel() % 8 == 0, "quick_gelu: the kernel handles 8 elements "
              "per lane, numel must be a multiple of 8, got ", x.numel());
  auto out = torch::empty_like(x);
  if (x.numel() == 0) return out;
  airtc_quick_gelu_f16(h_ptr(x), h_ptr_mut(out), x.numel(), cur_stream());
  return out;
}

std::vector<torch::Tensor> safety_head(
    torch::Tensor cls, torch::Tensor ln_g, torch::Tensor ln_b,
    torch::Tensor proj_w, torch::Tensor concept, torch::Tensor concept_w,
    torch::Tensor special, torch::Tensor special_w, torch::Tensor adjust,
    torch::Tensor counters, double eps) {
  // cls: (B, hidden) f16 rows with unit element stride; the row stride is
  // free, so the tower's x[:, 0] runs zero-copy
  TORCH_CHECK(cls.is_cuda() && cls.dim() == 2 && cls.dtype() == torch::kHalf,
              "safety_head: cls must be a (B, hidden) float16 GPU tensor");
  const int64_t B = cls.size(0), hidden = cls.size(1);
  TORCH_CHECK(B >= 1 && B <= kIntMax, "safety_head: empty batch");
  TORCH_CHECK(hidden > 0 && hidden % 8 == 0,
              "safety_head: the kernel reads 8 channels per lane, hidden = ",
              hidden);
  TORCH_CHECK(cls.stride(1) == 1 && cls.stride(0) % 8 == 0 &&
                  aligned16(cls.data_ptr()),
              "safety_head: cls rows must be dense and start on 16-byte "
              "boundaries");
  check_operand(ln_g, cls, torch::kFloat, hidden, "safety_head: ln_g");
  check_operand(ln_b, cls, torch::kFloat, hidden, "safety_head: ln_b");
  check_operand(proj_w, cls, torch::kHalf, "safety_head: proj_w");
  TORCH_CHECK(proj_w.dim() == 2 && proj_w.size(1) == hidden &&
                  proj_w.size(0) >= 1,
              "safety_head: proj_w must be (proj, hidden)");
  TORCH_CHECK(aligned16(proj_w.data_ptr()),
              "safety_head: proj_w must start on a 16-byte boundary");
  const int64_t proj = proj_w.size(0);
  check_operand(concept, cls, torch::kFloat, "safety_head: concept");
  check_operand(special, cls, torch::kFloat, "safety_head: special");
  TORCH_CHECK(concept.dim() == 2 && concept.size(1) == proj &&
                  concept.size(0) >= 1 && special.dim() == 2 &&
                  special.size(1) == proj && special.size(0) >= 1,
              "safety_head: concept and special must be (n >= 1, proj)");
  const int64_t nc = concept.size(0), ns = special.size(0);
  check_operand(concept_w, cls, torch::kFloat, nc, "safety_head: concept_w");
  check_operand(special_w, cls, torch::kFloat, ns, "safety_head: special_w");
  check_operand(adjust, cls, torch::kFloat, B, "safety_head: adjust");
  check_operand(counters, cls, torch::kInt, B, "safety_head: counters");
  TORCH_CHECK(hidden + proj + ns + nc <= 15000,
              "safety_head: hidden + proj + table rows must fit 64 KB of LDS");
  auto flags = torch::empty({B}, cls.options().dtype(torch::kInt));
  auto scores = torch::empty({B, ns + nc}, cls.options().dtype(torch::kFloat));
  airtc_safety_head(h_ptr(cls), cls.stride(0), ln_g.data_ptr<float>(),
                    ln_b.data_ptr<float>(), h_ptr(proj_w),
                    special.data_ptr<float>(), special_w.data_ptr<float>(),
                    concept.data_ptr<float>(), concept_w.data_ptr<float>(),
                    adjust.data_ptr<float>(), counters.data_ptr<int>(),
                    flags.data_ptr<int>(), scores.data_ptr<float>(), (int)B,
                    (int)hidden, (int)proj, (int)ns, (int)nc, (float)eps,
                    cur_stream());
  return {flags, scores};
}

torch::Tensor blank_flagged_(torch::Tensor img, torch::Tensor flags) {
  CHECK_IN(img);
  TORCH_CHECK(img.dtype() == torch::kHalf,
              "blank_flagged_: img must be float16");
  TORCH_CHECK(img.dim() >= 1 && img.size(0) >= 1 && img.size(0) <= kGridYZ,
              "blank_flagged_: img must hold 1..", kGridYZ, " frames");
  const int64_t B = img.size(0);
  check_operand(flags, img, torch::kInt, B, "blank_flagged_: flags");
  const int64_t per = img.numel() / B;
  if (per == 0) return img;
  const int vec = per % 8 == 0 && aligned16(img.data_ptr()) ? 1 : 0;
  airtc_blank_flagged(h_ptr_mut(img), flags.data_ptr<int>(), (int)B, per, vec,
                      cur_stream());
  return img;
}

// --- per-row LoRA delta (lora.hip) --------------------------------------
struct LoraShape {
  int Bt, L, K, N, Ny, R, n_adapters;
};

LoraShape check_lora_delta(const torch::Tensor& y, const torch::Tensor& x,
                           const torch::Tensor& A, const torch::Tensor& B,
                           const torch::Tensor& row_adapter,
                           const torch::Tensor& row_scale,
                           int64_t col_offset) {
  check_operand(x, x, torch::kHalf, "lora_delta_: x");
  check_operand(y, x, torch::kHalf, "lora_delta_: y");
  check_operand(A, x, torch::kHalf, "lora_delta_: A");
  check_operand(B, x, torch::kHalf, "lora_delta_: B");
  TORCH_CHECK(x.dim() == 3 && y.dim() == 3 && A.dim() == 3 && B.dim() == 3,
              "lora_delta_: x (Bt, L, K), y (Bt, L, Ny), A (n, R, K), "
              "B (n, N, R)");
  const int64_t Bt = x.size(0), L = x.size(1), K = x.size(2);
  const int64_t Ny = y.size(2), n = A.size(0), R = A.size(1), N = B.size(1);
  TORCH_CHECK(y.size(0) == Bt && y.size(1) == L,
              "lora_delta_: y must have x's batch and tokens, got ",
              y.sizes(), " for x ", x.sizes());
  TORCH_CHECK(A.size(2) == K, "lora_delta_: A must be (n, R, K=", K,
              "), got ", A.sizes());
  TORCH_CHECK(n >= 1 && B.size(0) == n && B.size(2) == R,
              "lora_delta_: B must be (n=", n, ", N, R=", R, "), got ",
              B.sizes());
  check_operand(row_adapter, x, torch::kInt, Bt, "lora_delta_: row_adapter");
  check_operand(row_scale, x, torch::kFloat, Bt, "lora_delta_: row_scale");
  TORCH_CHECK(Bt >= 1 && Bt <= kGridYZ && L >= 1,
              "lora_delta_: 1..", kGridYZ, " rows of at least one token");
  TORCH_CHECK(R == 16 || R == 32 || R == 64,
              "lora_delta_: R must be 16, 32 or 64, got ", R);
  TORCH_CHECK(K >= 32 && K % 32 == 0, "lora_delta_: K % 32 != 0, got ", K);
  TORCH_CHECK(N >= 16 && N % 16 == 0, "lora_delta_: N % 16 != 0, got ", N);
  TORCH_CHECK(col_offset >= 0 && col_offset % 16 == 0,
              "lora_delta_: col_offset % 16 != 0, got ", col_offset);
  TORCH_CHECK(col_offset + N <= Ny, "lora_delta_: columns [", col_offset,
              ", ", col_offset + N, ") do not fit y's ", Ny);
  // y is read and written four columns (8 bytes) at a time
  TORCH_CHECK(Ny % 4 == 0, "lora_delta_: Ny % 4 != 0, got ", Ny);
  TORCH_CHECK(x.numel() <= kIntMax && y.numel() <= kIntMax &&
                  A.numel() <= kIntMax && B.numel() <= kIntMax,
              "lora_delta_: x, y, A and B must each hold fewer than 2^31 "
              "values");
  TORCH_CHECK(aligned16(x.data_ptr()) && aligned16(A.data_ptr()) &&
                  aligned16(B.data_ptr()) &&
                  ((uintptr_t)y.data_ptr() & 7) == 0,
              "lora_delta_: x, A, B must be 16-byte and y 8-byte aligned");
  return {(int)Bt, (int)L, (int)K, (int)N, (int)Ny, (int)R, (int)n};
}

torch::Tensor lora_delta_(torch::Tensor y, torch::Tensor x, torch::Tensor A,
                          torch::Tensor B, torch::Tensor row_adapter,
                          torch::Tensor row_scale, int64_t col_offset) {
  const LoraShape d =
      check_lora_delta(y, x, A, B, row_adapter, row_scale, col_offset);
  const int rc = airtc_lora_delta(
      h_ptr(x), h_ptr_mut(y), h_ptr(A), h_ptr(B), row_adapter.data_ptr<int>(),
      row_scale.data_ptr<float>(), d.Bt, d.L, d.K, d.N, d.Ny, d.R,
      (int)col_offset, d.n_adapters, cur_stream());
  TORCH_CHECK(rc == 0, "lora_delta_: the launcher refused the shape");
  return y;
}

// --- software H.264 baseline-intra codec (h264sw.cpp) -----------------
extern "C" {
void* airtc_h264enc_create(int w, int h);
void airtc_h264enc_set_slices(void*, int n);
void airtc_h264enc_destroy(void*);
int airtc_h264enc_encode(void*, const uint8_t*, int qp, uint8_t*, int cap);
int airtc_h264enc_encode_ex(void*, const uint8_t*, int qp, int force_idr,
                            uint8_t*, int cap);
int airtc_h264enc_encode_yuv(void*, const uint8_t*, int qp, int force_idr,
                             uint8_t*, int cap);
void airtc_h264enc_set_mb_mode(void*, int m);
void airtc_h264_pred4(int, const uint8_t*, const uint8_t*, uint8_t, int, int,
                      int, uint8_t*);
void* airtc_h264dec_create();
void airtc_h264dec_destroy(void*);
int airtc_h264dec_decode(void*, const uint8_t*, int, uint8_t*, int, int*, int*);
int airtc_h264dec_decode_yuv(void*, const uint8_t*, int, uint8_t*, int, int*,
                             int*, int*);
void airtc_h264dec_dims(void*, int*, int*);
int airtc_h264sw_table_check();
}

class H264SwEncoder {
 public:
  H264SwEncoder(int w, int h, int slices = 4, int mb_mode = 0)
      : w_(w), h_(h) {
    handle_ = airtc_h264enc_create(w, h);
    TORCH_CHECK(handle_, "invalid encoder dimensions");
    airtc_h264enc_set_slices(handle_, slices);
    airtc_h264enc_set_mb_mode(handle_, mb_mode);
  }
  ~H264SwEncoder() {
    if (handle_) airtc_h264enc_destroy(handle_);
  }
  H264SwEncoder(const H264SwEncoder&) = delete;
  // keyframe=false emits a P frame (P_Skip + intra refresh) once a
  // reference exists; true (default) emits an IDR with in-band SPS/PPS
  pybind11::bytes encode(pybind11::bytes rgb, int qp, bool keyframe = true) {
    std::string s(rgb);
    TORCH_CHECK((int)s.size() == w_ * h_ * 3, "rgb buffer size mismatch");
    return run(s, qp, keyframe, /*yuv=*/false);
  }
  // same encode from tight I420 planes (w*h Y, then Cb, then Cr): the
  // colour conversion already happened, e.g. on the GPU
  pybind11::bytes encode_yuv(pybind11::bytes i420, int qp,
                             bool keyframe = true) {
    std::string s(i420);
    TORCH_CHECK(w_ % 2 == 0 && h_ % 2 == 0, "I420 needs even dimensions");
    TORCH_CHECK((int)s.size() == w_ * h_ * 3 / 2,
                "i420 buffer size mismatch");
    return run(s, qp, keyframe, /*yuv=*/true);
  }

 private:
  pybind11::bytes run(const std::string& s, int qp, bool keyframe, bool yuv) {
    std::vector<uint8_t> out((size_t)w_ * h_ * 6 + 4096);
    int n;
    {
      pybind11::gil_scoped_release nogil;
      n = (yuv ? airtc_h264enc_encode_yuv : airtc_h264enc_encode_ex)(
          handle_, (const uint8_t*)s.data(), qp, keyframe ? 1 : 0, out.data(),
          (int)out.size());
    }
    TORCH_CHECK(n > 0, "h264 encode failed rc=", n);
    return pybind11::bytes((const char*)out.data(), n);
  }

  void* handle_;
  int w_, h_;
};

class H264SwDecoder {
 public:
  H264SwDecoder() { handle_ = airtc_h264dec_create(); }
  ~H264SwDecoder() {
    if (handle_) airtc_h264dec_destroy(handle_);
  }
  H264SwDecoder(const H264SwDecoder&) = delete;
  // returns (rgb_bytes, w, h) or None (no frame in this AU / undecodable)
  pybind11::object decode(pybind11::bytes data) {
    std::string s(data);
    int w = 0, h = 0, is_yuv = 0;
    if (run(s, /*yuv=*/false, &w, &h, &is_yuv) != 1) return pybind11::none();
    return pybind11::make_tuple(
        pybind11::bytes((const char*)buf_.data(), (size_t)w * h * 3), w, h);
  }
  // same decode, picture handed out as tight I420 planes (no colour
  // conversion): (bytes, w, h, is_i420) or None. is_i420 is False, and the
  // bytes are RGB24 as from decode(), when w or h is odd
  pybind11::object decode_yuv(pybind11::bytes data) {
    std::string s(data);
    int w = 0, h = 0, is_yuv = 0;
    if (run(s, /*yuv=*/true, &w, &h, &is_yuv) != 1) return pybind11::none();
    const size_t n = is_yuv ? (size_t)w * h * 3 / 2 : (size_t)w * h * 3;
    return pybind11::make_tuple(pybind11::bytes((const char*)buf_.data(), n),
                                w, h, is_yuv != 0);
  }

 private:
  int call(const std::string& s, bool yuv, int* w, int* h, int* is_yuv) {
    if (yuv)
      return airtc_h264dec_decode_yuv(handle_, (const uint8_t*)s.data(),
                                      (int)s.size(), buf_.data(),
                                      (int)buf_.size(), w, h, is_yuv);
    return airtc_h264dec_decode(handle_, (const uint8_t*)s.data(),
                                (int)s.size(), buf_.data(), (int)buf_.size(),
                                w, h);
  }
  int run(const std::string& s, bool yuv, int* w, int* h, int* is_yuv) {
    pybind11::gil_scoped_release nogil;
    int rc = call(s, yuv, w, h, is_yuv);
    if (rc == -8) {  // output buffer too small: size from the parsed SPS
      int dw = 0, dh = 0;
      airtc_h264dec_dims(handle_, &dw, &dh);
      if (dw > 0 && dh > 0) {
        buf_.resize((size_t)dw * dh * 3);
        rc = call(s, yuv, w, h, is_yuv);
      }
    }
    return rc;
  }

  void* handle_;
  std::vector<uint8_t> buf_ = std::vector<uint8_t>((size_t)1024 * 1024 * 3);
};

// --- VCN hardware encode session (vcn.cpp; hardware-unvalidated, see the
// scope note there — gated behind AIRTC_VCN_EXPERIMENTAL in media/codec.py)
extern "C" {
void* airtc_vcn_enc_create(int w, int h, char* errbuf, int errlen);
void airtc_vcn_enc_destroy(void*);
int airtc_vcn_enc_encode(void*, const uint8_t*, int qp, uint8_t*, int cap);
}

class VcnEncoder {
 public:
  VcnEncoder(int w, int h) : w_(w), h_(h) {
    char err[256] = {0};
    handle_ = airtc_vcn_enc_create(w, h, err, sizeof(err));
    if (!handle_) throw std::runtime_error(std::string("VCN encode: ") + err);
  }
  ~VcnEncoder() {
    if (handle_) airtc_vcn_enc_destroy(handle_);
  }
  VcnEncoder(const VcnEncoder&) = delete;
  pybind11::bytes encode(pybind11::bytes rgb, int qp) {
    std::string s(rgb);
    TORCH_CHECK((int)s.size() == w_ * h_ * 3, "rgb buffer size mismatch");
    std::vector<uint8_t> out((size_t)w_ * h_ * 2 + 65536);
    int n;
    {
      pybind11::gil_scoped_release nogil;
      n = airtc_vcn_enc_encode(handle_, (const uint8_t*)s.data(), qp,
                               out.data(), (int)out.size());
    }
    TORCH_CHECK(n > 0, "VCN encode failed rc=", n);
    return pybind11::bytes((const char*)out.data(), n);
  }

 private:
  void* handle_;
  int w_, h_;
};

pybind11::bytes h264_sps_pps(int width, int height) {
  uint8_t buf[256];
  int n = airtc_h264_sps_pps(width, height, buf, sizeof(buf));
  TORCH_CHECK(n > 0, "sps/pps generation failed");
  return pybind11::bytes(reinterpret_cast<const char*>(buf), n);
}

pybind11::dict vcn_probe() {
  char buf[512];
  int rc = airtc_vcn_probe(buf, sizeof(buf));
  pybind11::dict d;
  d["available"] = rc >= 0;
  d["h264_decode"] = rc >= 0 && (rc & 1);
  d["h264_encode"] = rc >= 0 && (rc & 2);
  d["detail"] = std::string(buf);
  return d;
}

// fused LCM scheduler math (elementwise.hip): one kernel per scheduler op
// the two tensors of a scheduler op, (B, ...) f16 with rows of a multiple of
// 8 elements (one 16-byte access per lane); returns the row size, 0 when
// there is nothing to compute
long sched_rows(const torch::Tensor& x, const torch::Tensor& y,
                const char* op) {
  TORCH_CHECK(x.dim() >= 1, op, ": tensors must be (B, ...)");
  check_operand(x, x, torch::kHalf, op);
  check_operand(y, x, torch::kHalf, x.numel(), op);
  if (x.numel() == 0) return 0;
  const long per_b = x.numel() / x.size(0);
  TORCH_CHECK(per_b % 8 == 0, op, ": row size must be a multiple of 8, got ",
              per_b);
  return per_b;
}

// a per-batch-row coefficient array: (B,) f32 on x's device
const float* sched_coef(const torch::Tensor& c, const torch::Tensor& x,
                        const char* what) {
  check_operand(c, x, torch::kFloat, x.size(0), what);
  return c.data_ptr<float>();
}

torch::Tensor sched_add_noise(torch::Tensor x0, torch::Tensor noise,
                              torch::Tensor a, torch::Tensor bt) {
  const long per_b = sched_rows(x0, noise, "sched_add_noise");
  const float* ap = sched_coef(a, x0, "a");
  const float* bp = sched_coef(bt, x0, "bt");
  auto out = torch::empty_like(x0);
  if (per_b == 0) return out;
  airtc_sched_add_noise(h_ptr(x0), h_ptr(noise), ap, bp, h_ptr_mut(out), per_b,
                        x0.numel(), cur_stream());
  return out;
}

torch::Tensor sched_blend(torch::Tensor xt, torch::Tensor eps,
                          torch::Tensor a, torch::Tensor bt,
                          torch::Tensor c_out, torch::Tensor c_skip) {
  const long per_b = sched_rows(xt, eps, "sched_blend");
  sched_coef(a, xt, "a");
  sched_coef(bt, xt, "bt");
  sched_coef(c_out, xt, "c_out");
  sched_coef(c_skip, xt, "c_skip");
  auto out = torch::empty_like(xt);
  if (per_b == 0) return out;
  airtc_sched_blend(h_ptr(xt), h_ptr(eps), a.data_ptr<float>(),
                    bt.data_ptr<float>(), c_out.data_ptr<float>(),
                    c_skip.data_ptr<float>(), h_ptr_mut(out), per_b,
                    xt.numel(), cur_stream());
  return out;
}

// residual-CFG step (elementwise.hip): one launch, per-row f32 coefficients.
// mode 0 self / 1 initialize: coef = g-1 per row, stock is read and shifted
// in place; mode 2 full: coef = g per row, no stock.
torch::Tensor rcfg_apply(int64_t mode, torch::Tensor eps, torch::Tensor coef,
                         c10::optional<torch::Tensor> delta,
                         c10::optional<torch::Tensor> stock, int64_t fbs) {
  CHECK_IN(eps);
  CHECK_IN(coef);
  TORCH_CHECK(mode >= 0 && mode <= 2, "mode must be 0 (self), 1 (initialize) or 2 (full)");
  TORCH_CHECK(eps.dtype() == torch::kHalf && coef.dtype() == torch::kFloat);
  TORCH_CHECK(eps.dim() >= 1 && fbs >= 1);
  const long B = coef.numel();
  const long rows_in = mode == 0 ? B : (mode == 1 ? B + fbs : 2 * B);
  TORCH_CHECK(B >= 1 && eps.size(0) == rows_in, "eps has ", eps.size(0),
              " rows, mode ", mode, " with ", B, " coefficient rows needs ",
              rows_in);
  TORCH_CHECK(fbs <= B && B % fbs == 0, "fbs must divide the row count");
  const long per_b = eps.numel() / rows_in;
  auto shape = eps.sizes().vec();
  shape[0] = B;
  auto out = torch::empty(shape, eps.options());
  auto overlap = [](const torch::Tensor& a, const torch::Tensor& b) {
    const char* a0 = static_cast<const char*>(a.data_ptr());
    const char* b0 = static_cast<const char*>(b.data_ptr());
    return a0 < b0 + b.nbytes() && b0 < a0 + a.nbytes();
  };
  TORCH_CHECK(!overlap(out, eps), "out must not alias eps");
  const float* dp = nullptr;
  uint16_t* sp = nullptr;
  bool vec = per_b % 8 == 0 && aligned16(eps.data_ptr()) &&
             aligned16(out.data_ptr());
  if (mode != 2) {
    TORCH_CHECK(delta.has_value() && stock.has_value(),
                "self/initialize need delta and stock");
    CHECK_IN((*delta));
    CHECK_IN((*stock));
    TORCH_CHECK(delta->dtype() == torch::kFloat && delta->numel() == B,
                "delta must be f32 (B,)");
    TORCH_CHECK(stock->dtype() == torch::kHalf && stock->sizes() == out.sizes(),
                "stock must be f16 with the output's shape");
    TORCH_CHECK(!overlap(*stock, eps), "stock must not alias eps");
    TORCH_CHECK(!overlap(out, *stock), "out must not alias stock");
    dp = delta->data_ptr<float>();
    sp = h_ptr_mut(*stock);
    vec = vec && aligned16(sp);
  }
  if (out.numel() == 0) return out;
  airtc_rcfg_apply((int)mode, h_ptr(eps), sp, coef.data_ptr<float>(), dp,
                   h_ptr_mut(out), B, fbs, per_b, vec ? 1 : 0, cur_stream());
  return out;
}

// fp8 hardware probes (fp8.hip): raw MX MFMA tile + fused scale-converts
torch::Tensor fp8_mx_probe(torch::Tensor A, torch::Tensor B, int64_t sa,
                           int64_t sb) {
  CHECK_IN(A);
  CHECK_IN(B);
  TORCH_CHECK(A.dtype() == torch::kUInt8 && B.dtype() == torch::kUInt8);
  TORCH_CHECK(A.numel() == 2048 && B.numel() == 2048, "fragments are 2048B");
  auto draw = torch::empty({256}, A.options().dtype(torch::kFloat));
  airtc_fp8_mx_probe(A.data_ptr<uint8_t>(), B.data_ptr<uint8_t>(),
                     draw.data_ptr<float>(), (int)sa, (int)sb, cur_stream());
  return draw;
}

torch::Tensor fp8_quant_probe(torch::Tensor in16, double sa, int64_t variant) {
  CHECK_IN(in16);
  TORCH_CHECK(in16.dtype() == torch::kHalf && in16.numel() == 16);
  auto out = torch::empty({16}, in16.options().dtype(torch::kUInt8));
  airtc_fp8_quant_probe(h_ptr(in16), (float)sa, out.data_ptr<uint8_t>(),
                        (int)variant, cur_stream());
  return out;
}

pybind11::tuple fp8_cvt_probe(torch::Tensor fin, double scale,
                              torch::Tensor enc_in) {
  CHECK_IN(fin);
  CHECK_IN(enc_in);
  TORCH_CHECK(fin.dtype() == torch::kHalf && fin.numel() == 2);
  TORCH_CHECK(enc_in.dtype() == torch::kUInt8 && enc_in.numel() == 2);
  auto enc_out = torch::empty({2}, enc_in.options());
  auto dec_out = torch::empty({2}, fin.options());
  airtc_fp8_cvt_probe(h_ptr(fin), (float)scale, enc_out.data_ptr<uint8_t>(),
                      enc_in.data_ptr<uint8_t>(), h_ptr_mut(dec_out),
                      cur_stream());
  return pybind11::make_tuple(enc_out, dec_out);
}

}  // namespace

void airtc_register_dtls(pybind11::module_& m);  // dtls.cpp

// gemm_lt.cpp: x·Wᵀ + bias + residual as one hipBLASLt call
torch::Tensor airtc_linear_residual(const torch::Tensor& x,
                                    const torch::Tensor& weight,
                                    const c10::optional<torch::Tensor>& bias,
                                    const torch::Tensor& residual);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  airtc_register_dtls(m);
  m.def("linear_residual", &airtc_linear_residual,
        "x (...,K) · weight (N,K)ᵀ + bias (N,) + residual in one hipBLASLt "
        "call (bias epilogue, C = residual, beta = 1); contiguous f16, fp32 "
        "accumulation",
        pybind11::arg("x"), pybind11::arg("weight"), pybind11::arg("bias"),
        pybind11::arg("residual"));
  // how the error for a shape the library has no algorithm for begins
  m.attr("LT_NO_ALGORITHM") = "linear_residual: no hipBLASLt algorithm";
  m.def("conv2d", &conv2d,
        "implicit-GEMM MFMA conv2d (NHWC): (out, partials | None); "
        "stats_groups > 0 also asks for GroupNorm partials of the output for "
        "a consumer norm with that many groups",
        pybind11::arg("x"), pybind11::arg("w_perm"),
        pybind11::arg("bias") = pybind11::none(),
        pybind11::arg("cbias") = pybind11::none(),
        pybind11::arg("residual") = pybind11::none(), pybind11::arg("R"),
        pybind11::arg("S"), pybind11::arg("stride") = 1,
        pybind11::arg("pad") = 0, pybind11::arg("act") = 0,
        pybind11::arg("in_affine") = pybind11::none(),
        pybind11::arg("in_act") = 0, pybind11::arg("stats_groups") = 0,
        pybind11::arg("x2") = pybind11::none(),
        pybind11::arg("upsample2x") = false, pybind11::arg("pad_hi") = 0);
  m.def("conv2d_tinyic", &conv2d_tinyic,
        "tiny-IC conv (IC <= 4, K <= 36), lanes along OC (NHWC)",
        pybind11::arg("x"), pybind11::arg("w_tiny"),
        pybind11::arg("bias") = pybind11::none(),
        pybind11::arg("cbias") = pybind11::none(),
        pybind11::arg("residual") = pybind11::none(), pybind11::arg("R"),
        pybind11::arg("S"), pybind11::arg("stride") = 1,
        pybind11::arg("pad") = 0, pybind11::arg("act") = 0,
        pybind11::arg("pad_hi") = 0);
  m.def("group_norm_silu", &group_norm_silu, pybind11::arg("x"),
        pybind11::arg("groups"), pybind11::arg("gamma"), pybind11::arg("beta"),
        pybind11::arg("eps"), pybind11::arg("act"),
        pybind11::arg("partials") = pybind11::none());
  m.def("group_norm_silu_fp8", &group_norm_silu_fp8,
        "GN+act writing e4m3 codes (producer-side fp8 quantization)",
        pybind11::arg("x"), pybind11::arg("groups"), pybind11::arg("gamma"),
        pybind11::arg("beta"), pybind11::arg("eps"), pybind11::arg("act"),
        pybind11::arg("a_scale"),
        pybind11::arg("partials") = pybind11::none());
  m.def("group_norm_coeffs", &group_norm_coeffs,
        "(B,C,2) f32 affine pairs for the fused GN->conv input transform");
  m.def("layer_norm", &layer_norm);
  m.def("attention_bhlc", &attention_bhlc);
  m.def("silu", &silu);
  m.def("geglu", &geglu);
  m.def("add_act", &add_act);
  m.def("upsample2x", &upsample2x);
  m.def("sched_add_noise", &sched_add_noise,
        "fused q(x_t|x0) sample: a*x0 + b*noise (per-batch-row coeffs)");
  m.def("sched_blend", &sched_blend,
        "fused LCM step: c_out*(x_t - b*eps)/a + c_skip*x_t");
  m.def("rcfg_apply", &rcfg_apply,
        "residual-CFG step, per-row f32 coefficients; shifts stock in place");
  m.def("preprocess_u8", &preprocess_u8);
  m.def("postprocess_u8", &postprocess_u8);
  m.def("fit_resize_u8", &fit_resize_u8,
        "crop + antialiased resize of a u8 RGB frame into one slot");
  m.def("fit_resize_u8_i420", &fit_resize_u8_i420,
        "crop + antialiased resize of a u8 RGB frame into a whole I420 frame");
  m.def("rgb_u8_to_i420", &rgb_u8_to_i420,
        "(B,H,W,3) u8 RGB -> (B,3H/2,W) u8 I420 (BT.601 limited, integer)",
        pybind11::arg("x"), pybind11::arg("out") = pybind11::none());
  m.def("postprocess_i420", &postprocess_i420,
        "(B,H,W,3) f16 in [-1,1] -> (B,3H/2,W) u8 I420 in one kernel",
        pybind11::arg("img"), pybind11::arg("out") = pybind11::none());
  m.def("i420_to_rgb_u8", &i420_to_rgb_u8,
        "(B,3H/2,W) u8 I420 -> (B,H,W,3) u8 RGB",
        pybind11::arg("x"), pybind11::arg("out") = pybind11::none());
  m.def("canny_hint", &canny_hint,
        "(B,H,W,3) u8 RGB -> edge hint written into out (f16/f32); thr (B,2) "
        "i32 read on the device, hysteresis bounded to `reach` steps",
        pybind11::arg("frames"), pybind11::arg("thr"), pybind11::arg("reach"),
        pybind11::arg("out"));
  m.def("clip_patches", &clip_patches,
        "decoder image -> CLIP patch rows (resize, crop, normalise), one "
        "launch, into `out`");
  m.def("quick_gelu", &quick_gelu);
  m.def("safety_head", &safety_head,
        "class token -> (flags i32, scores f32); counters += flags");
  m.def("blank_flagged_", &blank_flagged_,
        "flagged frames -> -1, in place");
  m.def("lora_delta_", &lora_delta_, pybind11::arg("y"), pybind11::arg("x"),
        pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("row_adapter"),
        pybind11::arg("row_scale"), pybind11::arg("col_offset") = 0);
  m.def("conv2d_fp8", &conv2d_fp8,
        "fp8 e4m3 implicit-GEMM conv2d on the MX-scaled MFMA (NHWC)",
        pybind11::arg("x"), pybind11::arg("w_fp8"), pybind11::arg("dq"),
        pybind11::arg("a_scale"), pybind11::arg("bias") = pybind11::none(),
        pybind11::arg("cbias") = pybind11::none(),
        pybind11::arg("residual") = pybind11::none(), pybind11::arg("R"),
        pybind11::arg("S"), pybind11::arg("stride") = 1,
        pybind11::arg("pad") = 0, pybind11::arg("act") = 0,
        pybind11::arg("in_affine") = pybind11::none(),
        pybind11::arg("in_act") = 0, pybind11::arg("out_scale") = 0.0);
  m.def("fp8_mx_probe", &fp8_mx_probe,
        "raw-fragment v_mfma_scale_f32_16x16x128_f8f6f4 tile (layout probe)");
  m.def("fp8_quant_probe", &fp8_quant_probe,
        "conv kernel's exact 16-value activation encode (variant 0/1)");
  m.def("fp8_cvt_probe", &fp8_cvt_probe,
        "v_cvt_scalef32_pk_{fp8_f16,f16_fp8} semantics probe");
  m.def("vcn_probe", &vcn_probe, "probe the VCN VA-API stack");
  m.def("h264_sps_pps", &h264_sps_pps, "Annex-B SPS+PPS for (w, h)");
  m.def("h264sw_table_check", []() { return airtc_h264sw_table_check(); },
        "0 iff all CAVLC tables are prefix-free");
  pybind11::class_<H264SwEncoder>(m, "H264SwEncoder")
      .def(pybind11::init<int, int, int, int>(), pybind11::arg("w"),
           pybind11::arg("h"), pybind11::arg("slices") = 4,
           pybind11::arg("mb_mode") = 0)
      .def("encode", &H264SwEncoder::encode, pybind11::arg("rgb"),
           pybind11::arg("qp"), pybind11::arg("keyframe") = true,
           "RGB24 bytes + QP -> Annex-B (IDR, or P when keyframe=false)")
      .def("encode_yuv", &H264SwEncoder::encode_yuv, pybind11::arg("i420"),
           pybind11::arg("qp"), pybind11::arg("keyframe") = true,
           "tight I420 bytes + QP -> Annex-B, no colour conversion");
  m.def("h264_pred4",
        [](int mode, pybind11::bytes top, pybind11::bytes left, int tl,
           bool ht, bool hl, bool htl) {
          std::string t(top), l(left);
          TORCH_CHECK(t.size() == 8 && l.size() == 4, "t8/l4 sizes");
          uint8_t out[16];
          airtc_h264_pred4(mode, (const uint8_t*)t.data(),
                           (const uint8_t*)l.data(), (uint8_t)tl, ht, hl, htl,
                           out);
          return pybind11::bytes((const char*)out, 16);
        },
        "one 4x4 intra prediction (decoder path) for golden tests");
  pybind11::class_<H264SwDecoder>(m, "H264SwDecoder")
      .def(pybind11::init<>())
      .def("decode", &H264SwDecoder::decode,
           "Annex-B AU -> (rgb bytes, w, h) | None")
      .def("decode_yuv", &H264SwDecoder::decode_yuv,
           "Annex-B AU -> (i420 bytes, w, h, is_i420) | None");
  pybind11::class_<VcnEncoder>(m, "VcnEncoder")
      .def(pybind11::init<int, int>())
      .def("encode", &VcnEncoder::encode,
           "RGB24 bytes + QP -> Annex-B IDR via the VCN hardware encoder");
}
