"""Convs that read their operands where they lie: the pointwise tail (a
resnet's 1x1 shortcut as a second K segment), nearest-2x in the A-load
address, and the lanes-along-OC kernel of the 4-/3-channel conv_in layers.

Reference for every case: the f32 torch path on the same f16 inputs
(computed on the CPU).

Bounds:
- tail: folded max-abs error <= the unfused pair's max-abs error, measured in
  the same test, plus one f16 ulp at the output's largest magnitude. The fold
  sums the same products in f32 in another order and rounds once where the
  pair rounds the skip and then the sum, so it sits at or below the pair; the
  ulp covers the summation order.
- upsample (opt-in, AIRTC_CONV_UP=1): bit-equal to upsample_nearest2x_nhwc +
  conv2d_nhwc (same values, same K order).
- tiny IC: error <= the AIRTC_CONV_TINYIC=0 path's error plus one f16 ulp at
  the output's largest magnitude (both accumulate the same products in f32
  in the same (r, s, c) order).
- GroupNorm partials from a tail conv's finalize: f32 sums of <= 2^12 f16
  values in another order than torch's: relative 2^12 * 2^-24 < 1e-3 of the
  sum of magnitudes.
"""
import math

import pytest
import torch

from ai_rtc_agent_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().to(DEV)


def ulp16(mag: float) -> float:
    """One f16 ulp at magnitude mag (normal range)."""
    return 2.0 ** (math.floor(math.log2(max(mag, 2.0 ** -14))) - 10)


def cpu32(t):
    return None if t is None else t.detach().float().cpu()


def ref_conv(x, w, b, **kw):
    """f32 torch reference on the CPU from the same f16 inputs."""
    kw = {k: (cpu32(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    if kw.get("tail") is not None:
        kw["tail"] = tuple(cpu32(t) for t in kw["tail"])
    return ops.conv2d_nhwc(cpu32(x), cpu32(w), cpu32(b), **kw)


def err_vs(y, ref):
    return (y.float().cpu() - ref).abs().max().item()


# --------------------------------------------------------------------------
# tail
# --------------------------------------------------------------------------

TAIL_SHAPES = [
    (1, 8, 8, 64, 64, 128),    # BM64 split-K
    (2, 9, 9, 64, 96, 64),     # BM64 split-K, ragged M and OC
    (1, 8, 8, 32, 64, 96),     # BK=32
    (1, 48, 48, 64, 64, 64),   # M >= 2048: BM128
]


def tail_case(B, H, W, IC, OC, IC2, with_bias):
    x = rnd(B, H, W, IC, seed=IC + H)
    x2 = rnd(B, H, W, IC2, seed=IC2 + H + 1)
    w = rnd(OC, IC, 3, 3, seed=3, scale=1.0 / math.sqrt(9 * IC))
    w2 = rnd(OC, IC2, 1, 1, seed=4, scale=1.0 / math.sqrt(IC2))
    b = b2 = cb = None
    if with_bias:
        b = rnd(OC, seed=5, scale=0.1)
        b2 = rnd(OC, seed=6, scale=0.1)
        cb = rnd(B, OC, seed=7, scale=0.5)
    return x, x2, w, w2, b, b2, cb


def pair_by_hand(x, x2, w, w2, b, b2, cb, **kw):
    skip = ops.conv2d_nhwc(x2, w2, b2, 1, 0)
    return ops.conv2d_nhwc(x, w, b, residual=skip, channel_bias=cb, **kw)


@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias_cbias"])
def test_tail_vs_pair_and_torch(shape, with_bias):
    x, x2, w, w2, b, b2, cb = tail_case(*shape, with_bias)
    ref = ref_conv(x, w, b, channel_bias=cb, tail=(x2, w2, b2))
    y = ops.conv2d_nhwc(x, w, b, channel_bias=cb, tail=(x2, w2, b2))
    pair = pair_by_hand(x, x2, w, w2, b, b2, cb)
    e_fold, e_pair = err_vs(y, ref), err_vs(pair, ref)
    ulp = ulp16(ref.abs().max().item())
    print(f"tail {shape} bias={with_bias}: fold {e_fold:.3e} pair {e_pair:.3e} "
          f"ulp {ulp:.3e}")
    assert y.shape == pair.shape and y.dtype == torch.float16
    assert e_fold <= e_pair + ulp


def test_tail_stats_groups(monkeypatch):
    monkeypatch.setenv("AIRTC_FIN_STATS", "1")
    shape = (1, 8, 8, 64, 64, 128)
    x, x2, w, w2, b, b2, cb = tail_case(*shape, True)
    G = 32
    ref = ref_conv(x, w, b, channel_bias=cb, tail=(x2, w2, b2))
    y = ops.conv2d_nhwc(x, w, b, channel_bias=cb, tail=(x2, w2, b2),
                        stats_groups=G)
    pair = pair_by_hand(x, x2, w, w2, b, b2, cb)
    e_fold, e_pair = err_vs(y, ref), err_vs(pair, ref)
    ulp = ulp16(ref.abs().max().item())
    print(f"tail stats {shape}: fold {e_fold:.3e} pair {e_pair:.3e}")
    assert e_fold <= e_pair + ulp
    # split-K shape: the finalize hands the consumer norm its partials
    assert hasattr(y, "_airtc_gn_part")
    part, g, _ = y._airtc_gn_part
    assert g == G
    B, H, W, OC = y.shape
    yf = y.float().view(B, H * W, G, OC // G)
    tot = part.sum(dim=1).view(B, G, 2)
    mag = yf.abs().sum(dim=(1, 3))
    assert ((tot[..., 0] - yf.sum(dim=(1, 3))).abs() <= 1e-3 * mag + 1e-6).all()
    sq = (yf * yf).sum(dim=(1, 3))
    assert ((tot[..., 1] - sq).abs() <= 1e-3 * sq + 1e-6).all()


@pytest.mark.parametrize("shape", TAIL_SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_tail_switch_off_is_the_pair(shape, monkeypatch):
    x, x2, w, w2, b, b2, cb = tail_case(*shape, True)
    want = pair_by_hand(x, x2, w, w2, b, b2, cb)
    monkeypatch.setenv("AIRTC_CONV_TAIL", "0")
    y = ops.conv2d_nhwc(x, w, b, channel_bias=cb, tail=(x2, w2, b2))
    assert torch.equal(y, want)


# --------------------------------------------------------------------------
# nearest-2x in the A-load
# --------------------------------------------------------------------------

@pytest.mark.parametrize("src,oc", [
    ((1, 5, 7, 64), 64),
    ((2, 24, 24, 64), 64),   # M >= 2048
    ((1, 5, 7, 64), 96),
], ids=["5x7", "24x24", "oc96"])
def test_upsample_in_the_load_is_bit_equal(src, oc, monkeypatch):
    monkeypatch.setenv("AIRTC_CONV_UP", "1")  # opt-in
    x = rnd(*src, seed=src[1])
    w = rnd(oc, src[3], 3, 3, seed=8, scale=1.0 / math.sqrt(9 * src[3]))
    b = rnd(oc, seed=9, scale=0.1)
    y = ops.conv2d_nhwc(x, w, b, upsample2x=True)
    want = ops.conv2d_nhwc(ops.upsample_nearest2x_nhwc(x), w, b)
    assert y.shape == (src[0], 2 * src[1], 2 * src[2], oc)
    assert torch.equal(y, want)
    ref = ref_conv(x, w, b, upsample2x=True)
    assert err_vs(y, ref) <= 1e-2


# --------------------------------------------------------------------------
# tiny IC
# --------------------------------------------------------------------------

def tiny_case(shape, ic, oc, *, bias, cbias, residual, act, monkeypatch):
    B, H, W = shape
    x = rnd(B, H, W, ic, seed=H + ic)
    w = rnd(oc, ic, 3, 3, seed=10, scale=1.0 / math.sqrt(9 * ic))
    b = rnd(oc, seed=11, scale=0.1) if bias else None
    cb = rnd(B, oc, seed=12, scale=0.5) if cbias else None
    res = rnd(B, H, W, oc, seed=13) if residual else None
    kw = dict(channel_bias=cb, residual=res, act=act)
    ref = ref_conv(x, w, b, **kw)
    y = ops.conv2d_nhwc(x, w, b, **kw)
    monkeypatch.setenv("AIRTC_CONV_TINYIC", "0")
    old = ops.conv2d_nhwc(x, w, b, **kw)
    monkeypatch.delenv("AIRTC_CONV_TINYIC")
    e_new, e_old = err_vs(y, ref), err_vs(old, ref)
    ulp = ulp16(ref.abs().max().item())
    print(f"tiny {shape} {ic}->{oc} act={act}: new {e_new:.3e} old {e_old:.3e} "
          f"ulp {ulp:.3e}")
    assert y.shape == (B, H, W, oc) and y.dtype == torch.float16
    assert e_new <= e_old + ulp


def test_tiny_ic4_ragged(monkeypatch):
    tiny_case((1, 9, 9), 4, 64, bias=True, cbias=False, residual=False,
              act=ops.ACT_NONE, monkeypatch=monkeypatch)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_RELU], ids=["none", "relu"])
def test_tiny_ic4_unet_conv_in(bias, act, monkeypatch):
    tiny_case((2, 64, 64), 4, 320, bias=bias, cbias=False, residual=False,
              act=act, monkeypatch=monkeypatch)


def test_tiny_ic4_residual_and_channel_bias(monkeypatch):
    tiny_case((2, 64, 64), 4, 64, bias=True, cbias=True, residual=True,
              act=ops.ACT_NONE, monkeypatch=monkeypatch)


def test_tiny_ic3(monkeypatch):
    tiny_case((1, 16, 16), 3, 64, bias=True, cbias=False, residual=False,
              act=ops.ACT_NONE, monkeypatch=monkeypatch)


def test_tiny_ic4_accepts_stats_groups():
    # UNet conv_in passes the hint; shapes without a finalize ignore it
    x = rnd(1, 9, 9, 4, seed=20)
    w = rnd(64, 4, 3, 3, seed=21, scale=0.2)
    y = ops.conv2d_nhwc(x, w, None, stats_groups=32)
    assert torch.equal(y, ops.conv2d_nhwc(x, w, None))
    assert not hasattr(y, "_airtc_gn_part")


# --------------------------------------------------------------------------
# graph capture
# --------------------------------------------------------------------------

def test_upsample_conv_then_tail_conv_under_graph(monkeypatch):
    monkeypatch.setenv("AIRTC_CONV_UP", "1")  # opt-in
    x = rnd(1, 8, 8, 64, seed=30)
    x2 = rnd(1, 16, 16, 64, seed=31)
    wu = rnd(64, 64, 3, 3, seed=32, scale=1.0 / 24)
    w = rnd(64, 64, 3, 3, seed=33, scale=1.0 / 24)
    w2 = rnd(64, 64, 1, 1, seed=34, scale=1.0 / 8)
    b = rnd(64, seed=35, scale=0.1)

    def chain():
        h = ops.conv2d_nhwc(x, wu, None, upsample2x=True)
        return ops.conv2d_nhwc(h, w, b, tail=(x2, w2, b))

    eager = chain()  # also builds the weight packs before capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = chain()
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, out)
    assert torch.equal(first, eager)
