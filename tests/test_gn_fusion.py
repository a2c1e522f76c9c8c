"""CPU side of the finalize -> GroupNorm statistics fusion: the reference
path ignores the hint, and the bound the GPU test uses for fused vs unfused
holds for two f32 summation orders."""
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.models.unet import UNet2DCondition, UNetConfig


def test_stats_groups_ignored_on_cpu():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 8, 8, 32, generator=g)
    w = torch.randn(64, 32, 3, 3, generator=g) * 0.05
    cb = torch.randn(2, 64, generator=g)
    y0 = ops.conv2d_nhwc(x, w, None, channel_bias=cb)
    y1 = ops.conv2d_nhwc(x, w, None, channel_bias=cb, stats_groups=8)
    assert torch.equal(y0, y1)
    assert not hasattr(y1, "_airtc_gn_part")
    gamma, beta = torch.ones(64), torch.zeros(64)
    assert torch.equal(ops.group_norm_silu_nhwc(y0, 8, gamma, beta),
                       ops.group_norm_silu_nhwc(y1, 8, gamma, beta))


def test_tiny_unet_forward_unchanged_by_the_hint(monkeypatch):
    torch.manual_seed(0)
    cfg = UNetConfig.tiny()
    net = UNet2DCondition(cfg).eval()
    g = torch.Generator().manual_seed(1)
    sample = torch.randn(1, 8, 8, cfg.in_channels, generator=g)
    t = torch.tensor([500])
    ctx = torch.randn(1, 77, cfg.cross_attention_dim, generator=g)
    with torch.no_grad():
        y1 = net(sample, t, ctx)
    seen = []
    real = ops.conv2d_nhwc

    def no_hint(*a, stats_groups=None, **k):
        seen.append(stats_groups)
        return real(*a, **k)

    monkeypatch.setattr(ops, "conv2d_nhwc", no_hint)
    with torch.no_grad():
        y0 = net(sample, t, ctx)
    assert any(s for s in seen), "the UNet forward passes no group count down"
    assert torch.equal(y0, y1)


def test_summation_order_bound_holds_in_f32():
    """Fused and unfused statistics add the same f16 values in f32 in two
    different orders; the normalised f16 outputs then differ by at most one
    rounding: |a-b| <= 1e-4 + 2^-10 * max(|a|,|b|)."""
    g = torch.Generator().manual_seed(3)
    b, hw, c, groups = 2, 256, 320, 32
    cg = c // groups
    x = (torch.randn(b, hw, c, generator=g) * 1.5 + 0.7).half().float()
    gamma = torch.randn(c, generator=g) * 0.3 + 1.0
    beta = torch.randn(c, generator=g) * 0.2
    xg = x.reshape(b, hw, groups, cg)

    def seq_sum(t, dim):
        # strictly sequential f32 adds along dim
        acc = torch.zeros_like(t.select(dim, 0))
        for i in range(t.shape[dim]):
            acc = acc + t.select(dim, i)
        return acc

    def stats(order):
        if order == 0:    # pixels first, then the group's channels
            s = seq_sum(seq_sum(xg, 1), 2)
            q = seq_sum(seq_sum(xg * xg, 1), 2)
        else:             # channels first, 16 pixel chunks, then chunks
            xc = seq_sum(xg, 3).reshape(b, 16, hw // 16, groups)
            qc = seq_sum(xg * xg, 3).reshape(b, 16, hw // 16, groups)
            s = seq_sum(seq_sum(xc, 2), 1)
            q = seq_sum(seq_sum(qc, 2), 1)
        n = float(hw * cg)
        mean = s / n
        return mean, torch.rsqrt(q / n - mean * mean + 1e-5)

    outs = []
    for order in (0, 1):
        mean, rstd = stats(order)
        m = mean.repeat_interleave(cg, dim=1)[:, None, :]
        r = rstd.repeat_interleave(cg, dim=1)[:, None, :]
        y = (x - m) * r * gamma + beta
        outs.append(torch.nn.functional.silu(y).half().float())
    a, c2 = outs
    bound = 1e-4 + 2.0 ** -10 * torch.maximum(a.abs(), c2.abs())
    assert bool(((a - c2).abs() <= bound).all())
