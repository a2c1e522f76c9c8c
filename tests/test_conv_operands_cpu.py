"""conv2d_nhwc operands on the torch reference path: `tail=` (a pointwise
second K segment) and `upsample2x=` (nearest-2x in front of the conv) equal
the explicit compositions.

The reference path computes in f32 and rounds once, so against a composition
that is also kept in f32 the result is the same up to f32 summation order:
the bound is one rounding of the output dtype (f32 here: 1e-5 absolute on
O(1) values)."""
import torch
import torch.nn.functional as F

from ai_rtc_agent_amd import ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def test_tail_equals_sum_of_convs():
    x = rnd(2, 5, 6, 8, seed=1)
    x2 = rnd(2, 5, 6, 12, seed=2)
    w = rnd(7, 8, 3, 3, seed=3, scale=0.2)
    w2 = rnd(7, 12, 1, 1, seed=4, scale=0.2)
    b, b2 = rnd(7, seed=5), rnd(7, seed=6)
    cb = rnd(2, 7, seed=7)
    y = ops.conv2d_nhwc(x, w, b, channel_bias=cb, act=ops.ACT_SILU,
                        tail=(x2, w2, b2))
    main = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1)
    skip = F.conv2d(x2.permute(0, 3, 1, 2), w2, b2)
    want = F.silu((main + skip).permute(0, 2, 3, 1) + cb[:, None, None, :])
    assert y.shape == (2, 5, 6, 7)
    assert (y - want).abs().max().item() <= 1e-5


def test_tail_without_biases_and_with_residual():
    x = rnd(1, 4, 4, 8, seed=11)
    x2 = rnd(1, 4, 4, 8, seed=12)
    w = rnd(8, 8, 3, 3, seed=13, scale=0.2)
    w2 = rnd(8, 8, 1, 1, seed=14, scale=0.2)
    res = rnd(1, 4, 4, 8, seed=15)
    y = ops.conv2d_nhwc(x, w, None, residual=res, tail=(x2, w2, None))
    pair = ops.conv2d_nhwc(
        x, w, None,
        residual=ops.conv2d_nhwc(x2, w2, None, 1, 0, residual=res))
    assert (y - pair).abs().max().item() <= 1e-5


def test_upsample2x_equals_interpolate_then_conv():
    x = rnd(2, 3, 5, 8, seed=21)
    w = rnd(6, 8, 3, 3, seed=22, scale=0.2)
    b = rnd(6, seed=23)
    y = ops.conv2d_nhwc(x, w, b, upsample2x=True)
    up = ops.upsample_nearest2x_nhwc(x)
    assert up.shape == (2, 6, 10, 8)
    want = ops.conv2d_nhwc(up, w, b)
    assert y.shape == (2, 6, 10, 6)
    assert torch.equal(y, want)


def test_upsample2x_with_tail():
    x = rnd(1, 2, 3, 8, seed=31)
    x2 = rnd(1, 4, 6, 4, seed=32)
    w = rnd(5, 8, 3, 3, seed=33, scale=0.2)
    w2 = rnd(5, 4, 1, 1, seed=34, scale=0.2)
    y = ops.conv2d_nhwc(x, w, None, tail=(x2, w2, None), upsample2x=True)
    want = ops.conv2d_nhwc(ops.upsample_nearest2x_nhwc(x), w, None,
                           tail=(x2, w2, None))
    assert torch.equal(y, want)
