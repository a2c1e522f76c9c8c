"""CLIP safety checker on the CPU: the tower against transformers, the head
against a float64 transcription of the decision law, the checkpoint key map
against the published architecture, the preprocessing against PIL, and the
engine's gate end to end. Bounds and their provenance: _safety_ref.py."""
import os
import sys
import types

import pytest
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import EngineConfig
from ai_rtc_agent_amd.engine import StreamDiffusionEngine
from ai_rtc_agent_amd.models.load import (load_model_dir, load_safety_checker,
                                           safety_checker_key_map)
from ai_rtc_agent_amd.models.safety_clip import ClipSafetyChecker, ClipSafetyConfig

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _safety_ref as R  # noqa: E402


# ---------------------------------------------------------------------------
# tower and head
# ---------------------------------------------------------------------------
def _hf_vision(cfg, device=None):
    from transformers import CLIPVisionConfig, CLIPVisionModel

    hf_cfg = CLIPVisionConfig(
        hidden_size=cfg.hidden, intermediate_size=cfg.mlp,
        num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
        image_size=cfg.image, patch_size=cfg.patch,
        projection_dim=cfg.projection, hidden_act="quick_gelu",
        layer_norm_eps=cfg.eps)
    if device is None:
        return CLIPVisionModel(hf_cfg).eval()
    with torch.device(device):
        return CLIPVisionModel(hf_cfg)


def _checkpoint_prefix(hf):
    """What turns CLIPVisionModel's own keys into the checkpoint's: the
    checker holds it as `vision_model`, and transformers < 5 nests the
    transformer under a second `vision_model` (5.x serialises it flat, the
    published file is the nested form)."""
    nested = all(k.startswith("vision_model.") for k in hf.state_dict())
    return "vision_model." if nested else "vision_model.vision_model."


def test_tower_matches_transformers():
    cfg = R.TINY_CFG
    sd = R.random_state_dict(cfg, seed=1, scale=0.2)
    ours = R.checker_from(sd, cfg)
    hf = _hf_vision(cfg)
    prefix = _checkpoint_prefix(hf)
    res = hf.load_state_dict(
        {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)},
        strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    pixels = torch.randn(3, 3, cfg.image, cfg.image,
                         generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = hf(pixel_values=pixels).pooler_output
        got = ours.pooled(ClipSafetyChecker.patchify(pixels, cfg.patch))
    err = float((got - want).abs().max())
    print("pooler_output max abs diff", err)
    assert want.abs().mean() > 0.1  # a live comparison
    assert err <= 1e-5


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=str)
def test_head_follows_the_law(case):
    kw, flags, scores = R.head_case(*case)
    counters = torch.zeros(case[2], dtype=torch.int32)
    got_f, got_s = ops.safety_head(**kw, counters=counters)
    assert got_f.dtype == torch.int32 and got_s.dtype == torch.float32
    assert got_s.shape == (case[2], case[3] + case[4])
    assert float(scores.abs().min()) >= 10 * R.HEAD_TOL
    err = float((got_s.double() - scores).abs().max())
    print("score err", err)
    assert err <= R.HEAD_TOL
    assert torch.equal(got_f, flags)
    assert torch.equal(counters, flags)
    ops.safety_head(**kw, counters=counters)
    assert torch.equal(counters, 2 * flags)


def test_special_care_lifts_a_concept_over_zero():
    for case in ((64, 32, 1, 3, 17), (64, 32, 1, 1, 1)):
        kw, flags, scores = R.head_case(*case, hit=True)
        ns = case[3]
        # concept 0 sits in (-0.01, 0) before the lift and above zero after
        assert 0 < float(scores[0, ns]) < 0.01 and int(flags[0]) == 1
        f, s = ops.safety_head(**kw, counters=torch.zeros(1, dtype=torch.int32))
        assert int(f[0]) == 1 and float(s[0, ns]) > 0
        kw, flags, scores = R.head_case(*case, hit=False)
        assert -0.01 < float(scores[0, ns]) < 0 and int(flags[0]) == 0
        f, s = ops.safety_head(**kw, counters=torch.zeros(1, dtype=torch.int32))
        assert int(f[0]) == 0 and float(s[0, ns]) < 0


def test_quick_gelu_and_blank_torch_forms():
    x = torch.linspace(-6, 6, 101)
    assert torch.allclose(ops.quick_gelu(x), x * torch.sigmoid(1.702 * x))
    img = torch.rand(3, 4, 5, 3)
    keep = img.clone()
    out = ops.blank_flagged_(img, torch.tensor([0, 1, 0], dtype=torch.int32))
    assert out is img
    assert torch.equal(img[0], keep[0]) and torch.equal(img[2], keep[2])
    assert bool((img[1] == -1).all())


# ---------------------------------------------------------------------------
# checkpoint layout
# ---------------------------------------------------------------------------
def test_key_map_is_the_published_layout():
    cfg = ClipSafetyConfig()
    assert (cfg.image, cfg.patch, cfg.hidden, cfg.layers, cfg.heads, cfg.mlp,
            cfg.projection, cfg.concepts, cfg.special, cfg.eps) == \
        (224, 14, 1024, 24, 16, 4096, 768, 17, 3, 1e-5)
    hf = _hf_vision(cfg, device="meta")
    want = {_checkpoint_prefix(hf) + k: tuple(v.shape) for k, v in hf.state_dict().items()
            if not k.endswith("position_ids")}
    want.update({
        "visual_projection.weight": (768, 1024),
        "concept_embeds": (17, 768), "special_care_embeds": (3, 768),
        "concept_embeds_weights": (17,), "special_care_embeds_weights": (3,)})
    got = safety_checker_key_map(cfg)
    assert set(got) == set(want)
    assert all(tuple(got[k]) == want[k] for k in want)
    assert len(got) == 16 * 24 + 3 + 4 + 5
    # and the module really carries those names and shapes
    tiny = ClipSafetyChecker(R.TINY_CFG)
    own = {k: tuple(v.shape) for k, v in tiny.state_dict().items()}
    assert own == {k: tuple(v) for k, v in safety_checker_key_map(R.TINY_CFG).items()}


def test_loader_is_strict_both_ways():
    cfg = R.TINY_CFG
    sd = R.random_state_dict(cfg)
    ck = ClipSafetyChecker(cfg)
    assert ck.weights == "random"
    short = dict(sd)
    del short["visual_projection.weight"]
    with pytest.raises(ValueError, match="visual_projection.weight"):
        load_safety_checker(ck, short)
    with pytest.raises(ValueError, match="stowaway"):
        load_safety_checker(ck, dict(sd, stowaway=torch.zeros(1)))
    with pytest.raises(ValueError, match="concept_embeds"):
        load_safety_checker(ck, dict(sd, concept_embeds=torch.zeros(2, 2)))
    assert ck.weights == "random"
    pos = "vision_model.vision_model.embeddings.position_ids"
    assert load_safety_checker(ck, dict(sd, **{pos: torch.arange(5)[None]})) == len(sd)
    assert ck.weights == "loaded"
    assert torch.equal(ck.concept_embeds, sd["concept_embeds"])


def test_load_model_dir_round_trip(tmp_path, monkeypatch):
    from safetensors.torch import save_file

    cfg = R.TINY_CFG
    sd = R.random_state_dict(cfg, seed=5)
    monkeypatch.setenv("HF_HUB_CACHE", str(tmp_path / "empty"))
    ck = ClipSafetyChecker(cfg)
    holder = types.SimpleNamespace(safety_checker=ck, unet=None, vae=None)
    assert load_model_dir(holder, str(tmp_path)) is False and ck.weights == "random"
    os.makedirs(tmp_path / "safety_checker")
    save_file({k: v.contiguous() for k, v in sd.items()},
              str(tmp_path / "safety_checker" / "model.safetensors"))
    assert load_model_dir(holder, str(tmp_path)) is True
    assert ck.weights == "loaded"
    for k, v in ck.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # the checker's own repository in the HF cache is the second place
    snap = tmp_path / "hub" / "models--CompVis--stable-diffusion-safety-checker" \
        / "snapshots" / "abc"
    os.makedirs(snap)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(snap / "model.safetensors"))
    monkeypatch.setenv("HF_HUB_CACHE", str(tmp_path / "hub"))
    eng = _engine(checker=ClipSafetyChecker(cfg))
    assert eng.stats()["safety"]["weights"] == "loaded"


# ---------------------------------------------------------------------------
# preprocessing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", R.PIL_FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_clip_patches_u8_stage_against_pil(size):
    frame = R.u8_frame(*size, seed=size[0])
    pil, ours = R.pil_levels(frame, 224), R.our_levels(frame, 224)
    diff = int((pil - ours).abs().max())
    print("max level difference to PIL", size, diff)
    assert diff <= R.PIL_MAX_LEVEL_DIFF[size] + (1 if size != (224, 224) else 0)
    if size == (224, 224):
        assert torch.equal(ours, frame.to(torch.int64))
    # the op's result is that u8 stage through the table, as patches
    patches = ops.clip_patches(R.as_image(frame)[None], 224, 14)
    assert patches.dtype == torch.float16 and patches.shape == (1, 256, 588)
    assert torch.equal(R.patches_to_levels(patches, 224, 14)[0], ours)


def test_clip_filter_is_torch_antialiased_bicubic():
    import torch.nn.functional as F

    for h, w in ((64, 48), (300, 452), (226, 225)):
        frame = R.u8_frame(h, w, seed=h)
        nh, nw, top, left = ops.clip_geometry(h, w, 224)
        want = F.interpolate(frame.permute(2, 0, 1)[None].double(), size=(nh, nw),
                             mode="bicubic", antialias=True, align_corners=False)
        want = want[0, :, top:top + 224, left:left + 224].permute(1, 2, 0)
        got = ops.interface.clip_resize_reference(R.as_image(frame)[None], 224,
                                                  torch.float64)[0]
        assert float((got - want).abs().max()) < 1e-9
    assert ops.clip_geometry(300, 452, 224) == (224, 337, 0, 56)
    assert ops.clip_geometry(64, 48, 224) == (298, 224, 37, 0)


def test_clip_patches_order_and_arguments():
    import torch.nn.functional as F

    frame = R.u8_frame(28, 28, seed=3)
    patches = ops.clip_patches(R.as_image(frame)[None], 28, 14).float()
    lut = ops.interface.clip_lut("cpu").float()
    pixels = torch.stack([lut[c][frame[..., c].long()] for c in range(3)])[None]
    w = torch.randn(5, 3, 14, 14, generator=torch.Generator().manual_seed(4))
    want = F.conv2d(pixels, w, stride=14).flatten(2).transpose(1, 2)
    assert torch.allclose(patches @ w.reshape(5, -1).t(), want, atol=1e-4)
    assert torch.equal(ClipSafetyChecker.patchify(pixels, 14), patches)
    out = torch.empty(1, 4, 588, dtype=torch.float16)
    assert ops.clip_patches(R.as_image(frame)[None], 28, 14, out=out) is out
    for bad in (dict(img=torch.zeros(1, 7, 9, 3)), dict(img=torch.zeros(8, 8, 3)),
                dict(img=torch.zeros(1, 8, 8, 3), size=30)):
        with pytest.raises(ValueError):
            ops.clip_patches(**{"size": 28, "patch": 14, **bad})


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------
def _engine(weight=None, checker=None, fmt="rgb", fbs=1, **kw):
    if weight is not None:
        checker = ClipSafetyChecker(R.TINY_CFG)
        checker.concept_embeds_weights.data.fill_(weight)
    if checker is not None:
        kw.update(use_safety_checker=True, safety_checker="clip")
    cfg = EngineConfig(model_family="tiny", width=64, height=64, device="cpu",
                       use_hip_graph=False, use_lcm_lora=False,
                       output_format=fmt, frame_buffer_size=fbs, **kw)
    eng = StreamDiffusionEngine(cfg, safety_checker=checker)
    eng.prepare()
    return eng


FRAME = R.u8_frame(64, 64, seed=9)


def test_engine_gate_passes_and_blanks():
    plain = _engine()
    assert "safety" not in plain.stats()
    base = plain(FRAME)
    assert base.float().std() > 1  # a picture, not a constant
    assert torch.equal(_engine(2.0)(FRAME), base)
    assert int(_engine(-2.0)(FRAME).max()) == 0
    base420 = _engine(fmt="i420")(FRAME)
    assert torch.equal(_engine(2.0, fmt="i420")(FRAME), base420)
    black = ops.rgb_u8_to_i420(torch.zeros(64, 64, 3, dtype=torch.uint8))
    assert torch.equal(_engine(-2.0, fmt="i420")(FRAME), black)


def test_engine_per_slot_adjustment_counts_and_reset():
    eng = _engine(0.5, fbs=2)
    frames = torch.stack([FRAME, FRAME])
    first = eng(frames)
    assert first[0].float().std() > 1 and first[1].float().std() > 1
    st = eng.stats()["safety"]
    assert st["arch"] == "clip-vit" and st["weights"] == "random"
    assert st["adjustment"] == [0.0, 0.0] and st["frames_flagged"] == [0, 0]
    eng.update_safety(1.0, slot=1)
    out = eng(frames)
    assert out[0].float().std() > 1 and int(out[1].max()) == 0
    eng(frames)
    st = eng.stats()["safety"]
    assert st["adjustment"] == [0.0, 1.0] and st["frames_flagged"] == [0, 2]
    assert eng.slot_controls(1)["safety_adjustment"] == 1.0
    eng.reset_slot(1)
    out = eng(frames)
    assert out[1].float().std() > 1
    st = eng.stats()["safety"]
    assert st["adjustment"] == [0.0, 0.0] and st["frames_flagged"] == [0, 2]
    # every slot, and the default reset_slot restores, move together
    eng.update_safety(1.0)
    assert int(eng(frames).max()) == 0
    eng.reset_slot(0)
    assert eng.cfg.safety_adjustment == 1.0 and int(eng(frames).max()) == 0
    for bad in ("1", float("nan"), True):
        with pytest.raises(ValueError):
            eng.update_safety(bad)
    with pytest.raises(ValueError):
        _engine().update_safety(0.5)


def test_tiny_checker_is_still_the_default():
    from ai_rtc_agent_amd.models.safety import SafetyChecker

    eng = _engine(use_safety_checker=True)
    assert isinstance(eng.safety_checker, SafetyChecker)
    assert "safety" not in eng.stats()
    assert EngineConfig().safety_checker == "tiny" and EngineConfig().safety_adjustment == 0.0


# ---------------------------------------------------------------------------
# configuration surface
# ---------------------------------------------------------------------------
def test_config_validation(monkeypatch, capsys):
    with pytest.raises(ValueError, match="safety_checker"):
        EngineConfig(safety_checker="bogus")
    with pytest.raises(ValueError, match="safety_adjustment"):
        EngineConfig(safety_adjustment=float("inf"))
    monkeypatch.setenv("AIRTC_SAFETY_CHECKER", "clip")
    monkeypatch.setenv("AIRTC_SAFETY_ADJUSTMENT", "0.05")
    c = EngineConfig()
    assert (c.safety_checker, c.safety_adjustment) == ("clip", 0.05)
    monkeypatch.setenv("AIRTC_SAFETY_CHECKER", "bogus")
    with pytest.raises(ValueError):
        EngineConfig()
    from ai_rtc_agent_amd import agent

    monkeypatch.setattr(sys, "argv", ["agent", "--safety-checker", "bogus"])
    with pytest.raises(SystemExit) as e:
        agent.main()
    assert e.value.code == 2
    assert "--safety-checker" in capsys.readouterr().err


def test_runtime_config_cannot_reach_the_gate():
    """A publisher must not relax its own gate: the runtime config surface
    knows no safety key."""
    import inspect

    from ai_rtc_agent_amd import agent, pipeline

    for mod in (agent, pipeline):
        assert "update_safety" not in inspect.getsource(mod)
