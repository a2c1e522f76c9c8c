"""CPU half of the AutoencoderKL tests: the helpers of _vae_ref.py are
checked and measured here (the recorded constants must equal their
re-measurement), the module runs in f32 against the float64 reference, and
the loader, the engine switch, the config surface and the conv's
bottom/right-only padding are covered. See _vae_ref.py's docstring for the
bounds.
"""
import logging
import os
import types

import pytest
import torch
import torch.nn.functional as F

import _vae_ref as V
import _xfmr_ref as X
from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import EngineConfig
from ai_rtc_agent_amd.engine import StreamDiffusionEngine
from ai_rtc_agent_amd.engine.plan import plan_dir
from ai_rtc_agent_amd.models.load import (autoencoder_kl_key_map,
                                           load_autoencoder_kl, load_model_dir)
from ai_rtc_agent_amd.models.taesd import TinyVAE
from ai_rtc_agent_amd.models.vae_kl import (AutoencoderKLVAE, KLConfig,
                                             TINY_KL_CONFIG)

SIZED = [(c.name, h, w) for c in V.VAE_CASES for (h, w) in c.sizes]


def _vae(case, sd=None, **kw):
    vae = AutoencoderKLVAE(KLConfig(**case.kwargs), **kw)
    load_autoencoder_kl(vae, V.kl_state_dict(case) if sd is None else sd)
    return vae.eval()


# ---------------------------------------------------------------------------
# constants
# ---------------------------------------------------------------------------

def test_attention_d512_case_list_covers_the_issue():
    geos = {(c.lq, c.lk, c.b, c.h, c.layout) for c in V.ATTN512_CASES}
    for lq, lk in ((70, 77), (64, 64), (1, 1), (65, 130), (16, 1030)):
        assert (lq, lk, 2, 1, "plain") in geos
    assert any(g[4] == "qkv" for g in geos) and any(g[3] == 2 for g in geos)
    names = {c.name for c in V.ATTN512_CASES}
    assert len(names) == len(V.ATTN512_CASES) == 3 * len(geos)
    q, k, v = V.attn512_inputs(V.attn512_case("qkv-l70-normal"))
    assert q.stride(1) == 1536 and k.storage_offset() == 512
    assert v.storage_offset() == 1024 and not k.is_contiguous()


@pytest.fixture(scope="module")
def emulator_ratios():
    out = {}
    for c in V.ATTN512_CASES:
        o, A = V.attn512_reference(c.name)
        out[c.name] = X.attn_ratio(V.attn512_emulate(c), o, A)
    return out


def test_attention_d512_emulator_sets_the_constant(emulator_ratios):
    worst = max(emulator_ratios, key=emulator_ratios.get)
    print(f"emulator max ratio {emulator_ratios[worst]:.4f} at {worst}")
    assert abs(emulator_ratios[worst] - V.ATTN512_EMU_MAX) < 5e-3
    assert V.ATTN512_C == pytest.approx(2 * V.ATTN512_EMU_MAX, abs=5e-3)
    assert all(r <= V.ATTN512_C / 2 for r in emulator_ratios.values())


def test_attention_d512_bound_sees_a_wrong_kernel():
    """A dropped ragged tile, and a wave's 128 output columns left out."""
    for name in ("lq16-lk1030-normal", "lq65-lk130-offset"):
        c = V.attn512_case(name)
        q, k, v = V.attn512_inputs(c)
        o, A = V.attn512_reference(name)
        cut = (c.lk - 1) // V.ATTN512_KT * V.ATTN512_KT
        bad = X.attn_emulate(q, k[:, :cut], v[:, :cut], c.h, c.scale, V.ATTN512_KT)
        assert X.attn_ratio(bad, o, A) > V.ATTN512_C
        good = V.attn512_emulate(c).clone()
        good[..., 384:] = 0
        assert X.attn_ratio(good, o, A) > V.ATTN512_C


@pytest.mark.parametrize("name,H,W", SIZED)
def test_vae_reference_errors_are_the_recorded_ones(name, H, W):
    e32 = V.vae_ref_err(name, H, W, torch.float32, False)
    e16 = V.vae_ref_err(name, H, W, torch.float64, True)
    for side in ("encode", "decode"):
        print(f'("{name}", {H}, {W}, "{side}"): f32 ({e32[side][0]:.2e}, '
              f'{e32[side][1]:.2e}) f16 ({e16[side][0]:.2e}, {e16[side][1]:.2e})')
        for got, want in zip(e16[side], V.VAE16_ERR[(name, H, W, side)]):
            assert got == pytest.approx(want, rel=V.VAE16_RTOL)
        for got, want in zip(e32[side], V.VAE32_REF_ERR[(name, H, W, side)]):
            assert want / V.VAE32_FACTOR <= got <= want * V.VAE32_FACTOR


def test_reference_round16_is_f16_storage():
    case = V.vae_case("small")
    img, _ = V.vae_inputs(case, 16, 16)
    ref = V.kl_reference(V.kl_state_dict(case), case, round16=True)
    out = ref.encode(img)
    assert out.dtype == torch.float64 and torch.equal(out, out.half().double())


# ---------------------------------------------------------------------------
# the module in f32
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,H,W", SIZED)
def test_vae_f32_against_float64(name, H, W):
    case = V.vae_case(name)
    vae = _vae(case)
    img, lat = V.vae_inputs(case, H, W)
    e64, d64 = V.vae_reference(name, H, W)
    with torch.no_grad():
        got = {"encode": vae.encode(img), "decode": vae.decode(lat)}
    s = case.downscale
    assert got["encode"].shape == (2, H // s, W // s, 4)
    assert got["decode"].shape == (2, (H // s) * s, (W // s) * s, 3)
    for side, ref in (("encode", e64), ("decode", d64)):
        rms, mx = V.vae_err(got[side], ref)
        brms, bmx = V.VAE32_REF_ERR[(name, H, W, side)]
        print(f"{name} {H}x{W} {side}: rms {rms:.2e} (bound {4 * brms:.2e}) "
              f"max {mx:.2e} (bound {4 * bmx:.2e})")
        assert rms <= 4 * brms and mx <= 4 * bmx


def test_folded_encoder_tail_equals_unfolded():
    case = V.vae_case("small")
    vae = _vae(case)
    img, _ = V.vae_inputs(case, 16, 16)
    with torch.no_grad():
        folded = vae.encode(img)
        assert "_airtc_kl_tail" in ops.weight_cache_names()
        assert hasattr(vae, "_airtc_kl_tail")
        vae.fold_encoder_tail = False
        plain = vae.encode(img)
    # one linear map composed in f32 either way: K = 9 * 64 + 8 products
    assert (folded - plain).abs().max() <= 600 * 2.0 ** -24 * plain.abs().max()
    # the fold is a weight cache: new weights rebuild it
    vae.fold_encoder_tail = True
    with torch.no_grad():
        vae.quant_conv.bias.add_(1.0)
    ops.drop_weight_caches(vae)
    assert not hasattr(vae, "_airtc_kl_tail")
    with torch.no_grad():
        moved = vae.encode(img)
    assert (moved - folded - case.scaling_factor).abs().max() < 1e-5


def test_conv_pad_hi_cpu_path():
    g = torch.Generator().manual_seed(3)
    for h, w in ((9, 12), (16, 16)):
        x = torch.randn(2, h, w, 8, generator=g)
        wt = torch.randn(5, 8, 3, 3, generator=g)
        b = torch.randn(5, generator=g)
        got = ops.conv2d_nhwc(x, wt, b, stride=2, padding=0, pad_hi=1)
        ref = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1)), wt, b, stride=2)
        assert got.shape == (2, (h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1, 5)
        assert torch.equal(got, ref.permute(0, 2, 3, 1))
    assert torch.equal(ops.conv2d_nhwc(x, wt, b), ops.conv2d_nhwc(x, wt, b, pad_hi=0))
    with pytest.raises(ValueError, match="pad_hi"):
        ops.conv2d_nhwc(x, wt, b, pad_hi=-1)


# ---------------------------------------------------------------------------
# loader
# ---------------------------------------------------------------------------

def test_loader_round_trip_fills_every_parameter():
    case = V.vae_case("mid512")
    sd = V.kl_state_dict(case)
    vae = AutoencoderKLVAE(KLConfig(**case.kwargs))
    for p in vae.parameters():
        torch.nn.init.constant_(p, float("nan"))
    assert load_autoencoder_kl(vae, sd) == len(sd)
    assert not any(torch.isnan(p).any() for p in vae.parameters())
    a = vae.encoder.mid_block.attention
    p = "encoder.mid_block.attentions.0"
    assert torch.equal(a.to_qkv.weight[512:1024], sd[f"{p}.to_k.weight"])
    assert torch.equal(a.to_qkv.bias[1024:], sd[f"{p}.to_v.bias"])
    assert torch.equal(a.to_out.weight, sd[f"{p}.to_out.0.weight"])
    assert torch.equal(vae.encoder.down_blocks[0].downsample.weight,
                       sd["encoder.down_blocks.0.downsamplers.0.conv.weight"])
    assert torch.equal(vae.decoder.up_blocks[1].resnets[0].conv_shortcut.weight,
                       sd["decoder.up_blocks.1.resnets.0.conv_shortcut.weight"])
    layers, attns = autoencoder_kl_key_map(vae.cfg)
    assert 2 * len(layers) + 10 * len(attns) == len(sd)


def test_loader_takes_the_published_sd_vae_shape():
    """The default config's key map has the 248 tensors of the SD1.5 / SD2.1
    AutoencoderKL (diffusers 0.2x naming)."""
    layers, attns = autoencoder_kl_key_map(KLConfig())
    assert 2 * len(layers) + 10 * len(attns) == 248
    assert "decoder.up_blocks.2.resnets.0.conv_shortcut" in layers
    assert "encoder.down_blocks.3.downsamplers.0.conv" not in layers


def test_loader_legacy_attention_names():
    case = V.vae_case("small")
    img, _ = V.vae_inputs(case, 16, 16)
    new = _vae(case)
    old = _vae(case, V.kl_state_dict(case, legacy_attention=True))
    with torch.no_grad():
        assert torch.equal(new.encode(img), old.encode(img))


def test_loader_names_missing_and_surplus_keys():
    case = V.vae_case("small")
    sd = V.kl_state_dict(case)
    vae = AutoencoderKLVAE(KLConfig(**case.kwargs))
    short = dict(sd)
    del short["decoder.mid_block.attentions.0.to_k.bias"]
    with pytest.raises(ValueError, match="missing.*attentions.0.to_k.bias"):
        load_autoencoder_kl(vae, short)
    with pytest.raises(ValueError, match="unexpected.*stowaway"):
        load_autoencoder_kl(vae, dict(sd, stowaway=torch.zeros(1)))
    with pytest.raises(ValueError, match="shape mismatch.*quant_conv.weight"):
        load_autoencoder_kl(vae, dict(sd, **{"quant_conv.weight": torch.zeros(8, 4, 1, 1)}))


def test_load_model_dir_fills_the_kl_vae_or_skips(tmp_path, caplog):
    from safetensors.torch import save_file

    sd = V.kl_state_dict(V.VaeCase("tiny", TINY_KL_CONFIG.block_out_channels,
                                   TINY_KL_CONFIG.layers_per_block,
                                   TINY_KL_CONFIG.norm_num_groups, ()))
    os.makedirs(tmp_path / "vae")
    save_file(sd, str(tmp_path / "vae" / "diffusion_pytorch_model.safetensors"))
    kl = AutoencoderKLVAE(TINY_KL_CONFIG)
    holder = types.SimpleNamespace(vae=kl, unet=None, text_encoder=None)
    assert load_model_dir(holder, str(tmp_path)) is True
    assert torch.equal(kl.post_quant_conv.weight, sd["post_quant_conv.weight"])
    tiny = TinyVAE()
    before = tiny.encoder.conv_in.weight.clone()
    holder = types.SimpleNamespace(vae=tiny, unet=None, text_encoder=None)
    with caplog.at_level(logging.WARNING):
        assert load_model_dir(holder, str(tmp_path)) is False
    assert "full AutoencoderKL" in caplog.text
    assert torch.equal(tiny.encoder.conv_in.weight, before)


# ---------------------------------------------------------------------------
# engine, config, CLI
# ---------------------------------------------------------------------------

def test_engine_builds_the_kl_vae_and_runs_a_frame():
    cfg = EngineConfig(model_family="tiny", use_tiny_vae=False, device="cpu",
                       width=64, height=64, use_lcm_lora=False)
    eng = StreamDiffusionEngine(cfg)
    assert isinstance(eng.vae, AutoencoderKLVAE) and eng.vae.cfg == TINY_KL_CONFIG
    assert eng._fp8_vae["convs"] == []
    eng.prepare()
    frame = torch.randint(0, 256, (64, 64, 3), dtype=torch.uint8,
                          generator=torch.Generator().manual_seed(5))
    out = eng(frame)
    assert out.shape == (64, 64, 3) and out.dtype == torch.uint8
    tiny = StreamDiffusionEngine(EngineConfig(
        model_family="tiny", device="cpu", width=64, height=64, use_lcm_lora=False))
    assert isinstance(tiny.vae, TinyVAE)
    # the sd families get the checkpoint's own architecture
    assert KLConfig().block_out_channels == (128, 256, 512, 512)


def test_fp8_tier_stays_off_the_kl_vae():
    cfg = EngineConfig(model_family="tiny", use_tiny_vae=False, device="cpu",
                       width=64, height=64, use_lcm_lora=False, use_fp8=True)
    assert StreamDiffusionEngine(cfg)._fp8_vae == {"convs": [], "outs": []}


@pytest.mark.parametrize("family", ["sdxl", "tiny_xl"])
def test_full_vae_is_refused_for_sdxl(family):
    with pytest.raises(ValueError, match="float16"):
        EngineConfig(model_family=family, use_tiny_vae=False)
    assert EngineConfig(model_family=family).use_tiny_vae is True


def test_env_and_flag_parsing(monkeypatch):
    from ai_rtc_agent_amd.agent import build_parser, create_app

    monkeypatch.delenv("AIRTC_TINY_VAE", raising=False)
    assert EngineConfig().use_tiny_vae is True
    monkeypatch.setenv("AIRTC_TINY_VAE", "0")
    assert EngineConfig().use_tiny_vae is False
    assert EngineConfig(use_tiny_vae=True).use_tiny_vae is True
    monkeypatch.setenv("AIRTC_TINY_VAE", "1")
    assert EngineConfig().use_tiny_vae is True
    p = build_parser()
    assert p.parse_args([]).full_vae is False
    assert p.parse_args(["--full-vae"]).full_vae is True
    assert create_app(model_id="m", full_vae=True)["full_vae"] is True
    assert create_app(model_id="m")["full_vae"] is False


def test_plan_key_tells_the_vaes_apart(tmp_path):
    a = plan_dir("org/model", str(tmp_path))
    b = plan_dir("org/model", str(tmp_path), tiny_vae=False)
    assert a != b and a.endswith("engines--org--model")
    assert b.endswith("engines--org--model--full-vae")


def test_gpu_refusal_is_about_the_mid_width():
    assert ops.attention_serves(512) and ops.attention_serves(64)
    assert ops.attention_serves(40) and not ops.attention_serves(256)
    vae = AutoencoderKLVAE(KLConfig(block_out_channels=(32, 256), norm_num_groups=8))
    with pytest.raises(ValueError, match="256"):
        vae.check_gpu_support()
    AutoencoderKLVAE(KLConfig(**V.vae_case("mid512").kwargs)).check_gpu_support()


def test_attention_route_switch(monkeypatch):
    """AIRTC_VAE_ATTN=unfused is the same function by another route; anything
    else is refused."""
    case = V.vae_case("small")
    vae = _vae(case)
    img, _ = V.vae_inputs(case, 16, 16)
    monkeypatch.delenv("AIRTC_VAE_ATTN", raising=False)
    with torch.no_grad():
        base = vae.encode(img)
        monkeypatch.setenv("AIRTC_VAE_ATTN", "unfused")
        other = vae.encode(img)
        brms, bmx = V.VAE32_REF_ERR[("small", 16, 16, "encode")]
        assert (other - base).abs().max() <= 8 * bmx
        monkeypatch.setenv("AIRTC_VAE_ATTN", "sdpa")
        with pytest.raises(ValueError, match="AIRTC_VAE_ATTN"):
            vae.encode(img)
