"""linear + bias + residual as one hipBLASLt call (ops/csrc/gemm_lt.cpp).

Inputs are seeded: x, w ~ N(0,1)/sqrt(K), bias and residual ~ N(0,1).

Tolerance. The reference is x·Wᵀ + bias + residual in fp32 on the device.
F.linear(x, w, bias) + residual rounds to f16 twice (after the GEMM's
epilogue and after the add), the fused call once. A single rounding can land
on the other side of a tie from the double rounding, but never more than one
step away, so the fused call's max abs error may exceed the old path's by at
most one f16 ulp at the reference's largest magnitude,
2^(floor(log2 |v|max) - 10). Differences in fp32 summation order between the
two GEMM kernels are parts in 1e7 of the value and vanish under that ulp.

Everything else here is exact: a cached algorithm and a graph replay run the
same kernel on the same bits as the eager call.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from ai_rtc_agent_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (M, N, K): smallest problems that cover a square and a deep-K projection
# and an M that is no multiple of the 64-row tile
SHAPES = [(64, 320, 320), (256, 640, 2560), (48, 320, 1280)]


def fused(x, w, b, r):
    return ops.hip_ext().linear_residual(x, w, b, r)


def make(m, n, k, batch, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(batch, m, k, generator=g) / math.sqrt(k)).half().to(DEV)
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).half().to(DEV)
    b = torch.randn(n, generator=g).half().to(DEV)
    r = torch.randn(batch, m, n, generator=g).half().to(DEV)
    return x, w, b, r


@functools.lru_cache(maxsize=None)
def case(m, n, k, batch, has_bias):
    """Inputs, the fp32 reference and the old path's result: computed once,
    shared by the tests below, never written to."""
    x, w, b, r = make(m, n, k, batch, seed=m + n + k + batch)
    if not has_bias:
        b = None
    ref = x.float() @ w.float().T + r.float()
    if has_bias:
        ref = ref + b.float()
    old = F.linear(x, w, b) + r
    return x, w, b, r, ref, old


def f16_ulp(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(abs(v))) - 10)


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_error_vs_fp32_reference(m, n, k, has_bias, batch):
    x, w, b, r, ref, old = case(m, n, k, batch, has_bias)
    y = fused(x, w, b, r)
    assert y.shape == (batch, m, n) and y.dtype == torch.float16
    assert y.is_contiguous()
    err_new = (y.float() - ref).abs().max().item()
    err_old = (old.float() - ref).abs().max().item()
    ulp = f16_ulp(ref.abs().max().item())
    print(f"M={m} N={n} K={k} B={batch} bias={has_bias}: err_new={err_new:.3e} "
          f"err_old={err_old:.3e} ulp={ulp:.3e}")
    assert err_new <= err_old + ulp


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_second_call_is_bit_identical(m, n, k):
    """The second call runs on the cached descriptors and algorithm."""
    x, w, b, r, _, _ = case(m, n, k, 1, True)
    first = fused(x, w, b, r)
    second = fused(x, w, b, r)
    assert torch.equal(first, second)


def test_graph_capture_replays_bit_exact():
    m, n, k = SHAPES[0]
    sets = [make(m, n, k, 1, seed=s) for s in (11, 12, 13)]
    eager = [fused(*s) for s in sets]  # also the eager run before capture
    x, w, b, r = (t.clone() for t in sets[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fused(x, w, b, r)
    for s, want in zip(sets[1:], eager[1:]):
        for dst, src in zip((x, w, b, r), s):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_ops_linear_dispatch(monkeypatch):
    """ops.linear takes the one-call path for f16 GPU tensors with a
    residual, and the two-kernel path under AIRTC_LT_EPILOGUE=0."""
    x, w, b, r, _, old = case(*SHAPES[0], 2, True)
    monkeypatch.delenv("AIRTC_LT_EPILOGUE", raising=False)
    monkeypatch.delenv("AIRTC_FUSED_PROJ", raising=False)
    assert torch.equal(ops.linear(x, w, b, residual=r), fused(x, w, b, r))
    monkeypatch.setenv("AIRTC_LT_EPILOGUE", "0")
    assert torch.equal(ops.linear(x, w, b, residual=r), old)


def test_non_contiguous_residual_raises():
    x, w, b, r, _, _ = case(*SHAPES[0], 1, True)
    m, n = r.shape[1:]
    strided = torch.zeros(1, m, 2 * n, dtype=r.dtype, device=DEV)[..., :n]
    assert not strided.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        fused(x, w, b, strided)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.linear(x, w, b, residual=strided)


def test_fp32_input_raises():
    x, w, b, r, _, _ = case(*SHAPES[0], 1, True)
    with pytest.raises(RuntimeError, match="float16"):
        fused(x.float(), w, b, r)
    with pytest.raises(RuntimeError, match="float16"):
        fused(x, w, b.float(), r)


def test_shape_mismatch_raises():
    x, w, b, r, _, _ = case(*SHAPES[0], 1, True)
    with pytest.raises(RuntimeError, match="residual"):
        fused(x, w, b, r[:, :-1].contiguous())
    with pytest.raises(RuntimeError, match="bias"):
        fused(x, w, b[:-1].contiguous(), r)
