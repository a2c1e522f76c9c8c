"""Every tensor derived from a weight and hung on its parameter or module is
registered, drop_weight_caches removes all of them, and the next call
follows a weight changed in place.

Each caching route runs once at a small shape: MFMA conv, conv with a
pointwise tail, tiny-IC conv, pad-to-32 conv, fp8 conv, GroupNorm, LayerNorm,
linear with AIRTC_FUSED_PROJ=1 and a self-attention module (fused QKV).

Bound after the weight change, reference = the same op's torch path on the
CPU in f32 from the same f16 inputs: one f16 ulp at the reference's largest
magnitude for the f16 kernels (f32 math, one rounding, plus an f32 summation
order far below it); the fp8 conv against its CPU emulation within 2^-3 of
the largest magnitude (one e4m3 step of the activation grid at the top of
the range: the kernel's f16 staging may move a value across one code
boundary). What the test is about is that the result follows the NEW weight:
the old weight's result misses the same bound, which is asserted too.
"""
import math

import pytest
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.models.unet import CrossAttention, GroupNormSiLU, LayerNorm

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().to(DEV)


def ulp16(mag: float) -> float:
    return 2.0 ** (math.floor(math.log2(max(mag, 2.0 ** -14))) - 10)


def cpu32(t):
    if isinstance(t, tuple):
        return tuple(cpu32(v) for v in t)
    return t.detach().float().cpu() if torch.is_tensor(t) else t


class Conv(torch.nn.Module):
    def __init__(self, cin, cout, k=3, seed=0):
        super().__init__()
        self.weight = torch.nn.Parameter(rnd(cout, cin, k, k, seed=seed, scale=0.1))
        self.bias = torch.nn.Parameter(rnd(cout, seed=seed + 1))


class Lin(torch.nn.Module):
    def __init__(self, din, dout, seed=0):
        super().__init__()
        self.weight = torch.nn.Parameter(rnd(dout, din, seed=seed, scale=0.1))
        self.bias = torch.nn.Parameter(rnd(dout, seed=seed + 1))


def routes(monkeypatch):
    """name -> (module, run(module, to) -> output; `to` maps every tensor to
    the device/dtype under test, rel bound or None for one f16 ulp)."""
    monkeypatch.setenv("AIRTC_FUSED_PROJ", "1")
    x32, x3, x8 = rnd(1, 8, 8, 32, seed=1), rnd(1, 16, 16, 3, seed=2), rnd(1, 128, 128, 8, seed=3)
    x64, x2 = rnd(1, 8, 8, 64, seed=4), rnd(1, 8, 8, 64, seed=5)
    seq, res = rnd(1, 16, 64, seed=6), rnd(1, 16, 64, seed=7)
    sc = Conv(64, 32, k=1, seed=20)

    def conv(m, to, x, **kw):
        return ops.conv2d_nhwc(to(x), to(m.weight), to(m.bias), **kw)

    class Tail(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.shortcut = Conv(32, 32, seed=10), sc

    gn, ln = GroupNormSiLU(64).half().to(DEV), LayerNorm(64).half().to(DEV)
    attn = CrossAttention(64, 64, 2).half().to(DEV)
    return {
        "mfma": (Conv(32, 32, seed=30), lambda m, to: conv(m, to, x32), None),
        "tail": (Tail(), lambda m, to: ops.conv2d_nhwc(
            to(x32), to(m.conv.weight), to(m.conv.bias),
            tail=(to(x2), to(m.shortcut.weight), to(m.shortcut.bias))), None),
        "tinyic": (Conv(3, 32, seed=40), lambda m, to: conv(m, to, x3), None),
        "pad32": (Conv(8, 32, seed=50), lambda m, to: conv(m, to, x8), None),
        "fp8": (Conv(64, 64, seed=60), lambda m, to: ops.conv2d_fp8_nhwc(
            to(x64), to(m.weight), 0.02, to(m.bias)), 2.0 ** -3),
        "group_norm": (gn, lambda m, to: ops.group_norm_silu_nhwc(
            to(x64), m.groups, to(m.weight), to(m.bias), m.eps, False), None),
        "layer_norm": (ln, lambda m, to: ops.layer_norm(
            to(seq), to(m.weight), to(m.bias), m.eps), None),
        "fused_proj": (Lin(64, 64, seed=70), lambda m, to: ops.linear(
            to(seq), to(m.weight), to(m.bias), residual=to(res)), None),
    }, attn, seq


def found_attrs(module):
    """Every `_airtc_*` attribute on the parameters and every fused-projection
    attribute on the modules, by inspection (not through the registry)."""
    names = set()
    for m in module.modules():
        names |= {n for n in vars(m) if n in ("_wqkv", "_wkv", "_wq", "_wout")}
        for p in m.parameters(recurse=False):
            names |= {n for n in vars(p) if n.startswith("_airtc_")}
    return names


def test_caches_registered_dropped_and_rebuilt(monkeypatch):
    table, attn, seq = routes(monkeypatch)
    ident, cpu = (lambda t: t), cpu32
    tree = torch.nn.ModuleList([m for m, _, _ in table.values()] + [attn])

    old = {k: run(m, ident) for k, (m, run, _) in table.items()}
    attn_old = attn(seq)
    torch.cuda.synchronize()

    found = found_attrs(tree)
    expected = {"_airtc_wperm", "_airtc_b32", "_airtc_g32", "_airtc_w16",
                "_airtc_wpad32", "_airtc_wfp8", "_airtc_wdq", "_airtc_wtail",
                "_airtc_btail", "_airtc_wtiny", "_wqkv", "_wout"}
    assert expected <= found, expected - found
    assert found <= ops.weight_cache_names(), found - ops.weight_cache_names()

    ops.drop_weight_caches(tree)
    assert found_attrs(tree) == set()

    with torch.no_grad():
        for m, _, _ in table.values():
            for p in m.parameters():
                p.mul_(-0.5).add_(0.25)
        for p in attn.parameters():
            p.mul_(-0.5)  # no offset: keeps the softmax as flat as it was
    for k, (m, run, rel) in table.items():
        y = run(m, ident).float().cpu()
        ref = run(m, cpu).float()
        if ref.dtype != torch.float32 or y.shape != ref.shape:
            raise AssertionError(k)
        mag = ref.abs().max().item()
        bound = ulp16(mag) if rel is None else rel * mag
        err = (y - ref).abs().max().item()
        stale = (old[k].float().cpu() - ref).abs().max().item()
        print(k, "err", err, "bound", bound, "stale result err", stale)
        assert err <= bound, (k, err, bound)
        assert stale > bound, (k, stale, bound)
    # the attention module's fused projections follow the weights too: the
    # same module on the CPU in f32 (softmax in f32 on both sides; f16 QKV,
    # scores and output roundings along the chain: 2^-8 of the magnitude)
    y = attn(seq).float().cpu()
    ref_mod = CrossAttention(64, 64, 2)
    ref_mod.load_state_dict({k: v.float().cpu() for k, v in attn.state_dict().items()})
    ref = ref_mod(seq.float().cpu())
    mag = ref.abs().max().item()
    assert (y - ref).abs().max().item() <= mag * 2.0 ** -8
    assert (attn_old.float().cpu() - ref).abs().max().item() > mag * 2.0 ** -8
