// linear + bias + residual as ONE hipBLASLt call (host-side translation unit).
//
//   out = x · Wᵀ + bias + residual        f16 in/out, fp32 accumulation
//
// A GEMM computes D = alpha·A·B + beta·C anyway: C = residual with beta = 1
// and the library's bias epilogue replace the separate aten add (one launch
// and one read-read-write pass over the activation per projection), and the
// sum is rounded to f16 once instead of twice.
//
// Row-major out (M,N) is the column-major (N,M) problem Wᵀ·X:
//   A = weight, stored row-major (N,K) = column-major (K,N), ld K, opA = T
//   B = x,      stored row-major (M,K) = column-major (K,M), ld K, opB = N
//   C = residual, D = out: column-major (N,M), ld N
// The bias epilogue broadcasts along the rows of the column-major D, which
// is N: one bias value per output feature.
//
// One hipBLASLt per process: the extension links against the copy torch
// loads and uses the handle torch owns. Only the long-stable C entry points
// are used (matmul desc, matrix layout, preference, heuristic, matmul).
//
// hipGraph capture: descriptors and the chosen algorithm are cached per
// (device, M, N, K, has_bias) and the workspace per (device, stream), both
// for the life of the process, so a captured call allocates nothing but its
// output and replays with the pointers it was captured with. The eager
// warm-up frames fill the caches; a miss during capture only runs the
// host-side heuristic query, which is legal there.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>

#include <hipblaslt/hipblaslt.h>

#include <map>
#include <mutex>
#include <tuple>

namespace {

// upper bound handed to the heuristic; an algorithm that wants more is not
// offered. Split-K candidates at the largest shape in use (4096x320 f32
// partials, 5 MB each) fit several times over.
constexpr size_t kWorkspaceBytes = 32u << 20;

#define LT_CHECK(expr)                                                   \
  do {                                                                   \
    hipblasStatus_t st_ = (expr);                                        \
    TORCH_CHECK(st_ == HIPBLAS_STATUS_SUCCESS, "linear_residual: " #expr \
                " failed with hipblasStatus ", (int)st_);                \
  } while (0)

struct Plan {
  hipblasLtMatmulDesc_t desc = nullptr;
  hipblasLtMatrixLayout_t a = nullptr, b = nullptr, c = nullptr;
  hipblasLtMatmulAlgo_t algo;
  size_t workspace = 0;
};

using PlanKey = std::tuple<int, int64_t, int64_t, int64_t, bool>;

// Entries live for the process. Both maps are leaked on purpose: at exit the
// HIP runtime and torch's allocator may already be gone when static
// destructors run, and freeing device memory or descriptors then is unsafe.
std::mutex g_mu;
auto& g_plans = *new std::map<PlanKey, Plan>();
auto& g_workspace =
    *new std::map<std::pair<int, hipStream_t>, torch::Tensor>();

void destroy(Plan& p) {
  if (p.a) hipblasLtMatrixLayoutDestroy(p.a);
  if (p.b) hipblasLtMatrixLayoutDestroy(p.b);
  if (p.c) hipblasLtMatrixLayoutDestroy(p.c);
  if (p.desc) hipblasLtMatmulDescDestroy(p.desc);
  p = Plan();
}

// descriptors + heuristic for one problem; throws (and caches nothing) when
// the library offers no algorithm
void build_plan(hipblasLtHandle_t handle, Plan& p, int64_t M, int64_t N,
                int64_t K, bool has_bias) {
  LT_CHECK(hipblasLtMatmulDescCreate(&p.desc, HIPBLAS_COMPUTE_32F, HIP_R_32F));
  const int32_t op_t = HIPBLAS_OP_T, op_n = HIPBLAS_OP_N;
  LT_CHECK(hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_TRANSA,
                                           &op_t, sizeof(op_t)));
  LT_CHECK(hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_TRANSB,
                                           &op_n, sizeof(op_n)));
  if (has_bias) {
    const uint32_t epi = HIPBLASLT_EPILOGUE_BIAS;
    const int32_t bias_t = HIP_R_16F;
    LT_CHECK(hipblasLtMatmulDescSetAttribute(
        p.desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &epi, sizeof(epi)));
    LT_CHECK(hipblasLtMatmulDescSetAttribute(
        p.desc, HIPBLASLT_MATMUL_DESC_BIAS_DATA_TYPE, &bias_t,
        sizeof(bias_t)));
  }
  LT_CHECK(hipblasLtMatrixLayoutCreate(&p.a, HIP_R_16F, K, N, K));
  LT_CHECK(hipblasLtMatrixLayoutCreate(&p.b, HIP_R_16F, K, M, K));
  LT_CHECK(hipblasLtMatrixLayoutCreate(&p.c, HIP_R_16F, N, M, N));

  hipblasLtMatmulPreference_t pref = nullptr;
  LT_CHECK(hipblasLtMatmulPreferenceCreate(&pref));
  const uint64_t max_ws = kWorkspaceBytes;
  hipblasStatus_t st = hipblasLtMatmulPreferenceSetAttribute(
      pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &max_ws, sizeof(max_ws));
  hipblasLtMatmulHeuristicResult_t res;
  int found = 0;
  if (st == HIPBLAS_STATUS_SUCCESS)
    st = hipblasLtMatmulAlgoGetHeuristic(handle, p.desc, p.a, p.b, p.c, p.c,
                                         pref, 1, &res, &found);
  hipblasLtMatmulPreferenceDestroy(pref);
  // the text before the shape is what the Python caller matches on
  // (_C.LT_NO_ALGORITHM)
  TORCH_CHECK(st == HIPBLAS_STATUS_SUCCESS && found > 0 &&
                  res.state == HIPBLAS_STATUS_SUCCESS &&
                  res.workspaceSize <= kWorkspaceBytes,
              "linear_residual: no hipBLASLt algorithm for M=", M, " N=", N,
              " K=", K, has_bias ? " with bias" : " without bias",
              " (status ", (int)st, ", found ", found, ")");
  p.algo = res.algo;
  p.workspace = res.workspaceSize;
}

void check_f16(const torch::Tensor& t, const char* name,
               const torch::Tensor& x) {
  TORCH_CHECK(t.is_cuda(), "linear_residual: ", name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kHalf, "linear_residual: ", name,
              " must be float16");
  TORCH_CHECK(t.is_contiguous(), "linear_residual: ", name,
              " must be contiguous");
  TORCH_CHECK(t.device() == x.device(), "linear_residual: ", name,
              " is on another device than x");
}

}  // namespace

torch::Tensor airtc_linear_residual(const torch::Tensor& x,
                                    const torch::Tensor& weight,
                                    const c10::optional<torch::Tensor>& bias,
                                    const torch::Tensor& residual) {
  check_f16(x, "x", x);
  check_f16(weight, "weight", x);
  check_f16(residual, "residual", x);
  TORCH_CHECK(x.dim() >= 1 && weight.dim() == 2,
              "linear_residual: x must be (..., K), weight (N, K)");
  const int64_t N = weight.size(0), K = weight.size(1);
  TORCH_CHECK(K > 0 && N > 0 && x.size(-1) == K,
              "linear_residual: x (..., ", x.size(-1), ") against weight (", N,
              ", ", K, ")");
  const int64_t M = x.numel() / K;
  TORCH_CHECK(M > 0, "linear_residual: empty x");
  // int32-sized dimensions and element counts: what the library's kernels
  // index with
  TORCH_CHECK(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31) &&
                  M * N < (1LL << 31) && M * K < (1LL << 31) &&
                  N * K < (1LL << 31),
              "linear_residual: problem too large");
  TORCH_CHECK(residual.dim() == x.dim() && residual.size(-1) == N &&
                  residual.sizes().slice(0, x.dim() - 1) ==
                      x.sizes().slice(0, x.dim() - 1),
              "linear_residual: residual must have the output's shape");
  const void* bias_ptr = nullptr;
  if (bias.has_value()) {
    check_f16(*bias, "bias", x);
    TORCH_CHECK(bias->dim() == 1 && bias->size(0) == N,
                "linear_residual: bias must be (N,)");
    bias_ptr = bias->data_ptr();
  }

  const int dev = x.get_device();
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
  hipblasLtHandle_t handle = at::cuda::getCurrentCUDABlasLtHandle();
  auto out = torch::empty(residual.sizes(), x.options());

  // the lock covers the launch: the cached descriptor carries this call's
  // bias pointer until hipblasLtMatmul has read it
  std::lock_guard<std::mutex> lock(g_mu);
  const PlanKey key(dev, M, N, K, bias_ptr != nullptr);
  auto it = g_plans.find(key);
  if (it == g_plans.end()) {
    Plan p;
    try {
      build_plan(handle, p, M, N, K, bias_ptr != nullptr);
    } catch (...) {
      destroy(p);
      throw;
    }
    it = g_plans.emplace(key, p).first;
  }
  Plan& p = it->second;

  void* ws_ptr = nullptr;
  if (p.workspace > 0) {
    auto& ws = g_workspace[std::make_pair(dev, stream)];
    if (!ws.defined())
      ws = torch::empty({(int64_t)kWorkspaceBytes},
                        x.options().dtype(torch::kByte));
    ws_ptr = ws.data_ptr();
  }
  if (bias_ptr)
    LT_CHECK(hipblasLtMatmulDescSetAttribute(
        p.desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bias_ptr,
        sizeof(bias_ptr)));
  const float alpha = 1.f, beta = 1.f;
  LT_CHECK(hipblasLtMatmul(handle, p.desc, &alpha, weight.data_ptr(), p.a,
                           x.data_ptr(), p.b, &beta, residual.data_ptr(), p.c,
                           out.data_ptr(), p.c, &p.algo, ws_ptr, p.workspace,
                           stream));
  return out;
}
