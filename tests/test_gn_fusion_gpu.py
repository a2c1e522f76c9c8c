"""GroupNorm statistics fused into the split-K finalize, and the 16-byte
fast paths of the finalize and GroupNorm kernels.

Tolerances:
- GN vs f32 torch: 1e-2 max-abs, the bound of test_group_norm_silu_vs_torch.
- conv vs f32 torch: the bound of test_conv2d_vs_torch.
- fused vs unfused GN: the two paths differ only in f32 summation order of
  the statistics, which moves the pre-rounding value by parts in 1e6, so at
  most one f16 rounding apart: |a-b| <= 1e-4 + 2^-10 * max(|a|,|b|)
  (confirmed on the CPU in tests/test_gn_fusion.py).
- e4m3 apply: the kernel and the f32 reference differ by f32 rounding before
  the encode, so a code can only move to a neighbour: one e4m3 step is at
  most 1/8 of the larger magnitude (3 mantissa bits), or the subnormal step
  2^-9 * scale near zero. A flip needs the value within ~1e-5 relative of a
  rounding boundary whose spacing is ~6e-2 relative: well under 1 % of the
  elements.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from ai_rtc_agent_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().to(DEV)


def affine(c, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = (torch.randn(c, generator=g) * 0.3 + 1.0).float().to(DEV)
    beta = (torch.randn(c, generator=g) * 0.2).float().to(DEV)
    return gamma, beta


def gn_ref(x, groups, gamma, beta, eps, silu):
    y = F.group_norm(x.permute(0, 3, 1, 2).float(), groups, gamma, beta, eps)
    y = y.permute(0, 2, 3, 1)
    return F.silu(y) if silu else y


GN_SHAPES = [
    (2, 16, 16, 320, 32),   # Cg=10: 16 B vectors straddle groups
    (1, 8, 8, 1280, 32),
    (1, 4, 4, 960, 32),     # Cg=30
    (2, 6, 10, 64, 8),      # ragged pixel chunks
    (1, 2, 2, 640, 32),     # fewer pixels than thread rows
    (1, 8, 8, 36, 2),       # C % 8 != 0: the f16x2 fallback kernels
]


@pytest.fixture(autouse=True)
def fin_stats(monkeypatch):
    """Statistics from the finalize are opt-in (AIRTC_FIN_STATS=1, read per
    call; measured neutral end to end): the tests here run with them on."""
    monkeypatch.setenv("AIRTC_FIN_STATS", "1")


def test_fused_stats_are_opt_in(monkeypatch):
    monkeypatch.delenv("AIRTC_FIN_STATS")
    x = rnd(1, 8, 8, 64, seed=1)
    w = rnd(64, 64, 3, 3, seed=2, scale=0.05)
    y = ops.conv2d_nhwc(x, w, None, stats_groups=8)
    assert not hasattr(y, "_airtc_gn_part")
    monkeypatch.setenv("AIRTC_FIN_STATS", "1")
    y1 = ops.conv2d_nhwc(x, w, None, stats_groups=8)
    assert hasattr(y1, "_airtc_gn_part") and torch.equal(y, y1)


@pytest.fixture(params=["1", "0"], ids=["v8", "f16x2"])
def gn_fast(request, monkeypatch):
    """The 16 B GroupNorm kernels are opt-in (AIRTC_GN_FAST=1, read per
    call): every norm test runs on them and on the default kernels."""
    monkeypatch.setenv("AIRTC_GN_FAST", request.param)
    return request.param


@pytest.mark.parametrize("b,h,w,c,groups", GN_SHAPES)
@pytest.mark.parametrize("silu,eps", [(True, 1e-5), (False, 1e-6)])
def test_gn_fast_path_vs_torch(b, h, w, c, groups, silu, eps, gn_fast):
    x = rnd(b, h, w, c, seed=c + h)
    # a per-channel offset so group means differ and the table matters
    x = (x.float() + torch.linspace(-1, 1, c, device=DEV)).half()
    gamma, beta = affine(c, 7)
    y = ops.group_norm_silu_nhwc(x, groups, gamma, beta, eps=eps, silu=silu)
    ref = gn_ref(x, groups, gamma, beta, eps, silu)
    err = (y.float() - ref).abs().max().item()
    print(f"gn {b,h,w,c,groups} silu={silu}: max abs err {err:.3e}")
    assert y.shape == x.shape and y.dtype == torch.float16
    assert err <= 1e-2


@pytest.mark.parametrize("b,h,w,c,groups", GN_SHAPES)
def test_gn_fp8_apply_vs_roundtrip(b, h, w, c, groups, gn_fast):
    x = rnd(b, h, w, c, seed=c + h + 1)
    gamma, beta = affine(c, 8)
    ref = gn_ref(x, groups, gamma, beta, 1e-5, True)
    sa = ref.abs().max().item() / ops.FP8_MAX
    q = ops.group_norm_silu_nhwc(x, groups, gamma, beta, fp8_scale=sa)
    assert q.dtype == torch.uint8 and q.shape == x.shape
    dec = q.view(torch.float8_e4m3fn).float() * sa
    want = ops.fp8_roundtrip(ref, sa)
    diff = (dec - want).abs()
    step = torch.maximum(dec.abs(), want.abs()) / 8 + 2.0 ** -9 * sa
    frac = (diff > 0).float().mean().item()
    print(f"gn fp8 {b,h,w,c,groups}: {frac:.2e} of codes differ, "
          f"max diff {diff.max().item():.3e}")
    assert bool((diff <= step).all()), "a code moved by more than one step"
    assert frac < 0.01


def conv_ref(x, w, bias, cb, res, relu):
    y = F.conv2d(x.permute(0, 3, 1, 2).float(), w.float(),
                 None if bias is None else bias.float(), padding=1)
    y = y.permute(0, 2, 3, 1)
    if cb is not None:
        y = y + cb.float()[:, None, None, :]
    if res is not None:
        y = y + res.float()
    return F.relu(y) if relu else y


@pytest.mark.parametrize("b,h,ic,oc", [
    (1, 8, 1280, 1280),   # BM64 split path, OC % 4 == 0
    (1, 64, 64, 64),      # BM128 split path
    (1, 8, 64, 6),        # split-K with OC % 4 != 0: scalar finalize
])
def test_finalize_epilogue_vs_torch(b, h, ic, oc):
    assert _splits(b, h, oc, ic), "shape must take the split-K path"
    x = rnd(b, h, h, ic, seed=ic + oc)
    w = rnd(oc, ic, 3, 3, seed=1, scale=1.0 / math.sqrt(ic * 9))
    bias = rnd(oc, seed=2)
    cb = rnd(b, oc, seed=3)
    res = rnd(b, h, h, oc, seed=4)
    y = ops.conv2d_nhwc(x, w, bias, residual=res, channel_bias=cb,
                        act=ops.ACT_RELU)
    ref = conv_ref(x, w, bias, cb, res, True)
    err = (y.float() - ref).abs().max().item()
    tol = 2e-2 * max(1.0, math.sqrt(ic * 9) / 8)
    print(f"finalize {b,h,ic,oc}: max abs err {err:.3e} (tol {tol:.3e})")
    assert err <= tol


def _splits(b, h, oc, ic):
    """True when conv2d_nhwc(stats_groups=...) on this shape attaches
    partials for some valid group count, i.e. the finalize pass runs."""
    x = torch.zeros(b, h, h, ic, dtype=torch.float16, device=DEV)
    w = torch.zeros(oc, ic, 3, 3, dtype=torch.float16, device=DEV)
    if oc % 4 == 0:
        y = ops.conv2d_nhwc(x, w, None, stats_groups=oc // 4)
        return hasattr(y, "_airtc_gn_part")
    # no partials on the scalar path: ask the same geometry with OC = 8
    w8 = torch.zeros(8, ic, 3, 3, dtype=torch.float16, device=DEV)
    return hasattr(ops.conv2d_nhwc(x, w8, None, stats_groups=2),
                   "_airtc_gn_part")


FUSED_SHAPES = [
    (1, 8, 1280, 1280, 32),
    (2, 16, 320, 320, 32),
    (1, 64, 64, 64, 8),
]


def fused_chain(x, w, bias, cb, res, groups, gamma, beta, fuse):
    y = ops.conv2d_nhwc(x, w, bias, residual=res, channel_bias=cb,
                        stats_groups=groups if fuse else None)
    return y, ops.group_norm_silu_nhwc(y, groups, gamma, beta)


def chain_inputs(b, h, ic, oc, seed=0):
    x = rnd(b, h, h, ic, seed=seed + ic)
    w = rnd(oc, ic, 3, 3, seed=seed + 1, scale=1.0 / math.sqrt(ic * 9))
    bias = rnd(oc, seed=seed + 2)
    cb = rnd(b, oc, seed=seed + 3)
    res = rnd(b, h, h, oc, seed=seed + 4)
    return x, w, bias, cb, res


@pytest.mark.parametrize("b,h,ic,oc,groups", FUSED_SHAPES)
def test_fused_stats_match_unfused(b, h, ic, oc, groups, gn_fast):
    x, w, bias, cb, res = chain_inputs(b, h, ic, oc)
    gamma, beta = affine(oc, 9)
    y0, n0 = fused_chain(x, w, bias, cb, res, groups, gamma, beta, False)
    y1, n1 = fused_chain(x, w, bias, cb, res, groups, gamma, beta, True)
    assert not hasattr(y0, "_airtc_gn_part")
    part, g, _ = y1._airtc_gn_part
    assert g == groups and part.shape[0] == b * groups and part.shape[1] <= 64
    assert torch.equal(y0, y1), "conv output changed with stats_groups"
    a, c = n0.float(), n1.float()
    diff = (a - c).abs()
    bound = 1e-4 + 2.0 ** -10 * torch.maximum(a.abs(), c.abs())
    print(f"fused {b,h,ic,oc}: max |a-b| {diff.max().item():.3e}, "
          f"{(diff > 0).float().mean().item():.2e} of elements differ")
    assert bool((diff <= bound).all())
    # and the fused result is a correct GroupNorm of the conv output
    ref = gn_ref(y1, groups, gamma, beta, 1e-5, True)
    assert (c - ref).abs().max().item() <= 1e-2
    # a different group count must not pick the partials up
    gamma2, beta2 = affine(oc, 10)
    other = groups // 2
    n2 = ops.group_norm_silu_nhwc(y1, other, gamma2, beta2)
    ref2 = gn_ref(y1, other, gamma2, beta2, 1e-5, True)
    assert (n2.float() - ref2).abs().max().item() <= 1e-2


def test_unsplit_conv_attaches_nothing():
    x, w, bias, cb, res = chain_inputs(1, 64, 32, 1024)
    gamma, beta = affine(1024, 11)
    y, n = fused_chain(x, w, bias, cb, res, 32, gamma, beta, True)
    assert not hasattr(y, "_airtc_gn_part")
    ref = gn_ref(y, 32, gamma, beta, 1e-5, True)
    assert (n.float() - ref).abs().max().item() <= 1e-2


def test_fused_chain_deterministic_and_capturable():
    b, h, ic, oc, groups = 2, 16, 320, 320, 32
    x, w, bias, cb, res = chain_inputs(b, h, ic, oc)
    gamma, beta = affine(oc, 12)
    _, n0 = fused_chain(x, w, bias, cb, res, groups, gamma, beta, True)
    _, n1 = fused_chain(x, w, bias, cb, res, groups, gamma, beta, True)
    assert torch.equal(n0, n1), "fused chain is not run-to-run identical"

    xs = x.clone()
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        _, ng = fused_chain(xs, w, bias, cb, res, groups, gamma, beta, True)
    for seed in (40, 41):
        xin = rnd(b, h, h, ic, seed=seed)
        xs.copy_(xin)
        gph.replay()
        torch.cuda.synchronize()
        _, ne = fused_chain(xin, w, bias, cb, res, groups, gamma, beta, True)
        assert torch.equal(ng, ne), "graph replay differs from eager"
