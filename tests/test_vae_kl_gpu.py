"""GPU half of the AutoencoderKL tests: the d=512 attention kernel against
float64, bottom/right-only conv padding on every launcher that takes it, the
KL VAE in f16 against the float64 reference, and the engine with
use_tiny_vae=False. Bounds and case lists: _vae_ref.py.
"""
import pytest
import torch
import torch.nn.functional as F

import _vae_ref as V
import _xfmr_ref as X
from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import EngineConfig
from ai_rtc_agent_amd.engine import StreamDiffusionEngine
from ai_rtc_agent_amd.models.load import load_autoencoder_kl
from ai_rtc_agent_amd.models.taesd import TinyVAE
from ai_rtc_agent_amd.models.vae_kl import AutoencoderKLVAE, KLConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    e = ops.hip_ext()
    assert e is not None, "the HIP extension must be built"
    return e


# ---------------------------------------------------------------------------
# attention, one 512-wide head
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in V.ATTN512_CASES])
def test_attention_d512_against_float64(name, ext):
    c = V.attn512_case(name)
    q, k, v = V.attn512_inputs(c, "cuda")
    if c.layout == "qkv":
        assert q.stride(1) == 3 * V.ATTN512_D and not k.is_contiguous()
    got = ext.attention_bhlc(q, k, v, c.h, c.scale)
    torch.cuda.synchronize()
    assert got.shape == q.shape and got.dtype == torch.float16
    o, A = V.attn512_reference(name)
    ratio = X.attn_ratio(got, o, A)
    print(f"{name}: ratio {ratio:.4f} (bound {V.ATTN512_C})")
    assert not torch.isnan(got).any()
    assert ratio <= V.ATTN512_C


@pytest.mark.parametrize("name", ["lq70-lk77-normal", "qkv-l70-offset",
                                  "h2-lq70-lk77-peaked"])
def test_ops_attention_routes_d512(name):
    """ops.attention raised ValueError for d > 160 before the wide kernel."""
    c = V.attn512_case(name)
    q, k, v = V.attn512_inputs(c, "cuda")
    got = ops.attention(q, k, v, c.h)
    o, A = V.attn512_reference(name)
    ratio = X.attn_ratio(got, o, A)
    print(f"{name}: ratio {ratio:.4f}")
    assert ratio <= V.ATTN512_C


def test_attention_refusals_keep_their_words(ext):
    def qkv(d, h=1):
        return [torch.zeros(1, 16, d * h, dtype=torch.float16, device="cuda")
                for _ in range(3)]
    for d in (40, 192, 256, 1024):
        with pytest.raises(RuntimeError, match="head_dim") as ei:
            ext.attention_bhlc(*qkv(d), 1, 1.0)
        assert "512" in str(ei.value) and "160" in str(ei.value)
    with pytest.raises(ValueError, match="head_dim 256"):
        ops.attention(*qkv(256), 1)


# ---------------------------------------------------------------------------
# bottom/right-only padding, per launcher
# ---------------------------------------------------------------------------

def _pad_case(ic, oc, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, h, w, ic, generator=g).half()
    wt = (torch.randn(oc, ic, 3, 3, generator=g) / (3 * ic ** 0.5)).half()
    b = torch.randn(oc, generator=g).half()
    return x, wt, b


def _conv_tol(x, wt, b, stride, pad, pad_hi, ref):
    """f16 products are exact in f32, so both sides differ from the exact sum
    by K = 9 IC + 1 f32 roundings of magnitude sum |x||w| + |b| each, and the
    kernel's result by one f16 rounding (2^-25: half the subnormal spacing)."""
    mag = F.conv2d(F.pad(x.float().abs().permute(0, 3, 1, 2), (0, pad_hi, 0, pad_hi)),
                   wt.float().abs(), b.float().abs(), stride=stride, padding=pad)
    k = 9 * x.shape[-1] + 1
    return (2.0 ** -11 * ref.abs() + 2 * k * 2.0 ** -24 * mag.permute(0, 2, 3, 1)
            + 2.0 ** -25)


# launcher -> (IC, OC): mfma needs IC % 32 == 0, tinyic IC <= 4, direct the
# rest; large-spatial small-IC convs are padded to 32 channels and take mfma
PAD_LAUNCHERS = {"mfma": (32, 48), "mfma-ic64": (64, 64), "direct": (8, 24),
                 "tinyic": (3, 40)}


@pytest.mark.parametrize("hw", [(9, 12), (12, 9), (16, 16), (7, 7)])
@pytest.mark.parametrize("launcher", sorted(PAD_LAUNCHERS))
def test_conv_pad_hi_matches_cpu_path(launcher, hw):
    ic, oc = PAD_LAUNCHERS[launcher]
    x, wt, b = _pad_case(ic, oc, *hw, seed=ic * 100 + hw[0])
    for stride, pad, pad_hi in ((2, 0, 1), (1, 1, 2)):
        ref = ops.conv2d_nhwc(x.float(), wt.float(), b.float(), stride, pad,
                              pad_hi=pad_hi)
        own = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), (0, pad_hi, 0, pad_hi)),
                       wt.float(), b.float(), stride=stride, padding=pad)
        assert torch.equal(ref, own.permute(0, 2, 3, 1))
        got = ops.conv2d_nhwc(x.cuda(), wt.cuda(), b.cuda(), stride, pad,
                              pad_hi=pad_hi)
        assert got.shape == ref.shape
        err = (got.float().cpu() - ref).abs()
        tol = _conv_tol(x, wt, b, stride, pad, pad_hi, ref)
        assert (err <= tol).all(), (launcher, hw, stride, err.max().item())


def test_conv_pad_hi_large_spatial_small_ic():
    """IC < 32 at H*W >= 16384 is padded to 32 channels for the MFMA path:
    pad_hi travels with it."""
    x, wt, b = _pad_case(8, 16, 129, 128, seed=77)
    ref = ops.conv2d_nhwc(x.float(), wt.float(), b.float(), 2, 0, pad_hi=1)
    got = ops.conv2d_nhwc(x.cuda(), wt.cuda(), b.cuda(), 2, 0, pad_hi=1)
    assert got.shape == ref.shape == (2, 64, 64, 16)
    assert ((got.float().cpu() - ref).abs()
            <= _conv_tol(x, wt, b, 2, 0, 1, ref)).all()


def test_conv_pad_hi_refusals_come_from_the_binding(ext):
    x = torch.zeros(1, 4, 4, 32, dtype=torch.float16, device="cuda")
    w = torch.zeros(8, 9 * 32, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="pad_hi"):
        ext.conv2d(x=x, w_perm=w, R=3, S=3, stride=2, pad=0, pad_hi=-1)
    with pytest.raises(RuntimeError, match="2\\^29"):
        ext.conv2d(x=x, w_perm=w, R=3, S=3, stride=2, pad=0, pad_hi=(1 << 29) + 1)
    w7 = torch.zeros(8, 49 * 32, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="larger than the padded input 6x6"):
        ext.conv2d(x=x, w_perm=w7, R=7, S=7, stride=1, pad=0, pad_hi=2)


# ---------------------------------------------------------------------------
# the VAE in f16
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vaes():
    out = {}
    for case in V.VAE_CASES:
        vae = AutoencoderKLVAE(KLConfig(**case.kwargs))
        load_autoencoder_kl(vae, V.kl_state_dict(case))
        out[case.name] = vae.to("cuda", torch.float16).eval()
    return out


@pytest.mark.parametrize("name,H,W", [(c.name, h, w) for c in V.VAE_CASES
                                      for (h, w) in c.sizes])
def test_vae_f16_against_float64(name, H, W, vaes):
    case = V.vae_case(name)
    img, lat = V.vae_inputs(case, H, W)
    e64, d64 = V.vae_reference(name, H, W)
    with torch.no_grad():
        enc = vaes[name].encode(img.half().cuda())
        dec = vaes[name].decode(lat.half().cuda())
    torch.cuda.synchronize()
    for side, got, ref in (("encode", enc, e64), ("decode", dec, d64)):
        assert got.shape == ref.shape and got.dtype == torch.float16
        rms, mx = V.vae_err(got, ref)
        brms, bmx = V.VAE16_ERR[(name, H, W, side)]
        print(f"{name} {H}x{W} {side}: rms {rms:.3e} (bound {2 * brms:.3e}) "
              f"max {mx:.3e} (bound {2 * bmx:.3e})")
        assert rms <= 2 * brms and mx <= 2 * bmx


def test_vae_refuses_unserved_mid_width_on_the_gpu():
    with pytest.raises(ValueError, match="256"):
        AutoencoderKLVAE(KLConfig(block_out_channels=(32, 256), norm_num_groups=8),
                         device="cuda")
    vae = AutoencoderKLVAE(KLConfig(block_out_channels=(32, 256), norm_num_groups=8,
                                    layers_per_block=1)).to("cuda", torch.float16)
    with pytest.raises(ValueError, match="256"):
        vae.decode(torch.zeros(1, 4, 4, 4, dtype=torch.float16, device="cuda"))


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------

def _engine(**kw):
    args = dict(model_family="tiny", width=64, height=64, device="cuda",
                acceleration="hip", use_hip_graph=True, use_lcm_lora=False,
                t_index_list=[32], cfg_type="none")
    args.update(kw)
    eng = StreamDiffusionEngine(EngineConfig(**args))
    eng.prepare()
    return eng


def _frames(n):
    g = torch.Generator().manual_seed(91)
    return [torch.randint(0, 256, (64, 64, 3), generator=g, dtype=torch.uint8).cuda()
            for _ in range(n)]


def _run(eng, frames):
    out = []
    for f in frames:
        o = eng(f)
        eng.sync_output()
        out.append(o.clone())
    return out


def test_engine_full_vae_graph_matches_eager_and_repeats():
    frames = _frames(3)
    graph = _engine(use_tiny_vae=False)
    assert isinstance(graph.vae, AutoencoderKLVAE)
    a = _run(graph, frames)
    b = _run(_engine(use_tiny_vae=False, use_hip_graph=False), frames)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == (64, 64, 3) and x.dtype == torch.uint8
        assert torch.equal(x, y), f"captured replay differs from eager at frame {i}"
    # the same frames through a second captured engine: bit-identical replays
    c = _run(_engine(use_tiny_vae=False), frames)
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_engine_tiny_vae_is_unchanged_by_the_switch():
    frames = _frames(2)
    base = _run(_engine(), frames)
    _run(_engine(use_tiny_vae=False), frames)
    again = _engine(use_tiny_vae=True)
    assert isinstance(again.vae, TinyVAE)
    assert all(torch.equal(x, y) for x, y in zip(base, _run(again, frames)))
