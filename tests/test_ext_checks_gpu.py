"""The conv, GroupNorm and elementwise bindings refuse malformed operands on
the host: every case below raises RuntimeError from the binding's own checks,
and a well-formed call made straight after returns the right values (a call
that had reached a kernel with such operands would have read or written out
of bounds).

Shapes are 8x8x32 (8x8x64 for the fp8 conv, which needs IC % 64 == 0; 8x8x4
for the tiny-IC conv).

Bounds of the well-formed calls, reference = the f32 torch path on the CPU
from the same f16 inputs:
- conv, GroupNorm (no activation), silu, sched_blend: one f16 ulp at the
  reference's largest magnitude. The kernels compute in f32 and round once to
  f16 (half an ulp); what is left of the ulp covers the f32 summation order
  (K = 288 products, 288 * 2^-24 relative), the one-pass variance over 128
  values, the kernels' exp and the blend's multiply by 1/a where torch
  divides, all orders of magnitude below 2^-11 relative.
- fp8 conv: compared against the binding's own result on the same inputs
  before the malformed call (bit-equal); its accuracy is test_fp8_gpu's
  subject.
- upsample2x: bit-equal (a copy).
"""
import math

import pytest
import torch

from ai_rtc_agent_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, W, C, OC = 1, 8, 8, 32, 32


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def ulp16(mag: float) -> float:
    return 2.0 ** (math.floor(math.log2(max(mag, 2.0 ** -14))) - 10)


def close(y, ref):
    ref = ref.float().cpu()
    err = (y.float().cpu() - ref).abs().max().item()
    bound = ulp16(ref.abs().max().item())
    assert err <= bound, (err, bound)


@pytest.fixture(scope="module")
def ext():
    return ops.hip_ext()


# --- conv ------------------------------------------------------------------

def conv_operands(kind):
    """Well-formed keyword arguments of one conv binding."""
    ic = {"conv2d": C, "conv2d_fp8": 64, "conv2d_tinyic": 4}[kind]
    x = rnd(B, H, W, ic, seed=1)
    w = rnd(OC, ic, 3, 3, seed=2, scale=0.1)
    kw = dict(x=x, bias=rnd(OC, seed=3, dtype=torch.float32),
              cbias=rnd(B, OC, seed=4), residual=rnd(B, H, W, OC, seed=5),
              R=3, S=3, stride=1, pad=1, act=ops.ACT_NONE)
    if kind == "conv2d":
        kw["w_perm"] = w.permute(0, 2, 3, 1).reshape(OC, -1).contiguous()
    elif kind == "conv2d_tinyic":
        kw["w_tiny"] = ops.interface._tiny_pack(w)
    else:
        q, scale = ops.quantize_weight_fp8(w)
        kw.update(w_fp8=q, dq=(scale * 0.05).contiguous(), a_scale=0.05)
    return kw, w


def run_conv(ext, kind, kw):
    y = getattr(ext, kind)(**kw)
    return y[0] if kind == "conv2d" else y


def bad_bias(kw):
    kw["bias"] = kw["bias"][:-1].contiguous()


def bad_cbias(kw):
    kw["cbias"] = kw["cbias"].reshape(-1)[:-1].contiguous()


def cpu_bias(kw):
    kw["bias"] = kw["bias"].cpu()


def stride0(kw):
    kw["stride"] = 0


def x_3d(kw):
    kw["x"] = kw["x"][0]


def big_kernel(kw):
    # 11x11 on the 8x8 input padded to 10x10
    kw.update(R=11, S=11, w_perm=rnd(OC, 11 * 11 * C, seed=6))


CONV_CASES = [(k, f) for k in ("conv2d", "conv2d_fp8", "conv2d_tinyic")
              for f in (bad_bias, bad_cbias, cpu_bias, stride0, x_3d)]
CONV_CASES.append(("conv2d", big_kernel))


@pytest.mark.parametrize("kind,breaker", CONV_CASES,
                         ids=[f"{k}-{f.__name__}" for k, f in CONV_CASES])
def test_conv_refuses(ext, kind, breaker):
    kw, w = conv_operands(kind)
    good = run_conv(ext, kind, kw)
    bad = dict(kw)
    breaker(bad)
    with pytest.raises(RuntimeError):
        run_conv(ext, kind, bad)
    again = run_conv(ext, kind, kw)
    torch.cuda.synchronize()
    assert torch.equal(again, good)
    if kind != "conv2d_fp8":
        ref = ops.conv2d_nhwc(
            kw["x"].float().cpu(), w.float().cpu(), kw["bias"].cpu(),
            residual=kw["residual"].float().cpu(),
            channel_bias=kw["cbias"].float().cpu())
        close(again, ref)


# --- GroupNorm -------------------------------------------------------------

def gn_operands():
    return (rnd(B, H, W, C, seed=7), rnd(C, seed=8, dtype=torch.float32),
            rnd(C, seed=9, dtype=torch.float32))


def strided_gamma(x, g, b):
    return x, 8, rnd(2 * C, seed=8, dtype=torch.float32)[::2], b


def short_gamma(x, g, b):
    return x, 8, g[:-1].contiguous(), b


def groups_not_dividing(x, g, b):
    return x, 5, g, b


def odd_channels_per_group(x, g, b):
    return x, C, g, b


GN_BREAKERS = (strided_gamma, short_gamma, groups_not_dividing,
               odd_channels_per_group)


@pytest.mark.parametrize("breaker", GN_BREAKERS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("binding", ["group_norm_coeffs", "group_norm_silu",
                                     "group_norm_silu_fp8"])
def test_group_norm_refuses(ext, binding, breaker):
    def call(x, groups, g, b):
        if binding == "group_norm_coeffs":
            return ext.group_norm_coeffs(x, groups, g, b, 1e-5)
        if binding == "group_norm_silu":
            return ext.group_norm_silu(x, groups, g, b, 1e-5, ops.ACT_NONE)
        return ext.group_norm_silu_fp8(x, groups, g, b, 1e-5, ops.ACT_NONE,
                                       0.05)

    x, g, b = gn_operands()
    with pytest.raises(RuntimeError):
        call(*breaker(x, g, b))
    y = call(x, 8, g, b)
    torch.cuda.synchronize()
    xc, gc, bc = x.float().cpu(), g.cpu(), b.cpu()
    if binding == "group_norm_coeffs":
        ref = ops.group_norm_coeffs(xc, 8, gc, bc)
        # f32 pairs from f32 statistics of 128 values in another order:
        # 128 * 2^-24 = 8e-6 relative on s, and the same times |gamma| * rstd
        # (< 8 here) absolute on t = beta - mean * s
        assert torch.allclose(y.cpu(), ref, rtol=1e-4, atol=1e-4)
    elif binding == "group_norm_silu":
        close(y, ops.group_norm_silu_nhwc(xc, 8, gc, bc, silu=False))
    else:
        # codes of the f16-exact path: each decodes within one e4m3 step
        # (2^-3 relative, 2^-9 * scale at the bottom) of the reference
        ref = ops.group_norm_silu_nhwc(xc, 8, gc, bc, silu=False)
        dec = y.cpu().view(torch.float8_e4m3fn).float() * 0.05
        tol = ref.abs().clamp(max=448 * 0.05) * 2.0 ** -3 + 0.05 * 2.0 ** -9
        assert ((dec - ref.clamp(-448 * 0.05, 448 * 0.05)).abs() <= tol).all()


# --- elementwise -----------------------------------------------------------

def test_silu_refuses_12_elements(ext):
    with pytest.raises(RuntimeError):
        ext.silu(rnd(12))
    x = rnd(B, H, W, C, seed=10)
    y = ext.silu(x)
    torch.cuda.synchronize()
    close(y, torch.nn.functional.silu(x.float().cpu()))


def test_upsample2x_refuses_f32(ext):
    x = rnd(B, H, W, C, seed=11)
    with pytest.raises(RuntimeError):
        ext.upsample2x(x.float())
    y = ext.upsample2x(x)
    torch.cuda.synchronize()
    ref = x.cpu().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(y.cpu(), ref)


def test_sched_blend_refuses_cpu_coefficients(ext):
    xt, eps = rnd(2, H, W, C, seed=12), rnd(2, H, W, C, seed=13)
    co = [torch.tensor(v, dtype=torch.float32, device=DEV)
          for v in ([0.9, 0.8], [0.4, 0.6], [0.7, 0.5], [0.3, 0.5])]
    with pytest.raises(RuntimeError):
        ext.sched_blend(xt, eps, co[0].cpu(), *co[1:])
    y = ext.sched_blend(xt, eps, *co)
    torch.cuda.synchronize()
    close(y, ops.sched_blend(xt.float().cpu(), eps.float().cpu(),
                             *[c.cpu() for c in co]))
