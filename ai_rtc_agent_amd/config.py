"""Configuration surface.

Mirrors the reference's three config mechanisms:
CLI flags (reference agent.py:441-455), environment variables
(reference docs/environment.md:3-25, Dockerfile:54-56, lib/tracks.py:17-18),
and the runtime API (POST /config + datachannel JSON — reference
agent.py:398-412). Pipeline hyperparameter defaults follow the reference's
canonical config (reference lib/pipeline.py:11-14, lib/wrapper.py:46-65).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import List, Optional


def _env_bool(name: str, default: bool = False) -> bool:
    v = os.environ.get(name)
    if v is None:
        return default
    return v.strip().lower() not in ("", "0", "false", "no", "off")


def _env_int(name: str, default: int) -> int:
    v = os.environ.get(name)
    return int(v) if v not in (None, "") else default


def _env_float(name: str, default: float) -> float:
    v = os.environ.get(name)
    return float(v) if v not in (None, "") else default


# ---------------------------------------------------------------------------
# Environment variable surface (parity list)
# ---------------------------------------------------------------------------
# AUTH_TOKEN / WEBHOOK_URL           -> webhook events (utils/events.py)
# TURN_* (replaces TWILIO_*)         -> ICE/TURN provisioning (media/ice.py)
# WARMUP_FRAMES / DROP_FRAMES        -> track adapter (media/tracks.py)
# ENGINES_CACHE (was TRT_ENGINES_CACHE) -> kernel-plan/graph cache dir
# CIVITAI_CACHE / HF_HOME / HF_HUB_CACHE -> model asset caches
# VCN_ENC / VCN_DEC (was NVENC/NVDEC) -> hardware codec toggles
# VCN_ENC_PRESET / VCN_ENC_TUNING_INFO / VCN_ENC_{DEFAULT,MIN,MAX}_BITRATE
#                                     -> encoder tunables (5-knob parity with
#                                        NVENC_* in reference docs/environment.md:17-25)
# AIRTC_FIT_MODE (cover|contain|stretch) -> EngineConfig.fit_mode, how frames
#                                        of another resolution are fitted
# AIRTC_OUTPUT_SIZE (engine|source)  -> EngineConfig.output_size: return each
#                                        frame at the engine's size, or at
#                                        the size its session published
# AIRTC_OUTPUT_MAX_SIDE (pixels)     -> EngineConfig.output_max_side: cap on
#                                        the longer side of a returned frame
#                                        (0 = none)
# AIRTC_MEDIA_YUV (0|1)              -> media_yuv(): the media plane and the
#                                        engine exchange I420 frames instead
#                                        of packed RGB (codec plane I/O, GPU
#                                        colour conversion); also the default
#                                        of EngineConfig.output_format
# AIRTC_RUNTIME_GUIDANCE (0|1)       -> EngineConfig.runtime_guidance: keep
#                                        the RCFG step in the captured graph
#                                        so guidance can be raised at runtime
# AIRTC_CONTROLNET_PROCESSOR (none|canny) -> EngineConfig.controlnet_processor:
#                                        what turns the live frame into the
#                                        ControlNet's hint
# AIRTC_CONTROLNET_SCALE (float)     -> EngineConfig.controlnet_scale
# AIRTC_CANNY_LOW / AIRTC_CANNY_HIGH  -> EngineConfig.canny_low / canny_high,
#                                        hysteresis thresholds on the L1
#                                        gradient magnitude (0..2040)
# AIRTC_CANNY_REACH (0..32)           -> EngineConfig.canny_reach: how many
#                                        3x3 steps a weak edge may lie from a
#                                        strong one
# AIRTC_SAFETY_CHECKER (tiny|clip)    -> EngineConfig.safety_checker: which
#                                        checker use_safety_checker builds;
#                                        clip = the reference's CLIP ViT-L/14
#                                        StableDiffusionSafetyChecker. The
#                                        agent switches the checker on when
#                                        this (or --safety-checker) is set
# AIRTC_SAFETY_ADJUSTMENT (float)     -> EngineConfig.safety_adjustment: added
#                                        to every clip score, positive is
#                                        stricter
# AIRTC_TINY_VAE (0|1)                -> EngineConfig.use_tiny_vae: 1 (default)
#                                        = TAESD; 0 = the checkpoint's full
#                                        AutoencoderKL (models/vae_kl.py):
#                                        sharper decode at about a third of the
#                                        frame rate. sd15 / sd21 only
# AIRTC_LORA_ADAPTERS (0..64)         -> EngineConfig.lora_adapters: capacity
#                                        of the per-session adapter bank; 0
#                                        (default) = the feature is off
# AIRTC_LORA_ADAPTER_FILES            -> NAME=PATH[:SCALE],... the adapters the
#                                        agent loads into bank indices 0, 1, ...
#                                        at start-up (--lora-adapter)
# AIRTC_LORA_MAX_RANK (1..64)         -> EngineConfig.lora_max_rank: largest
#                                        adapter rank the bank accepts


def engines_cache_dir() -> str:
    return os.environ.get(
        "ENGINES_CACHE", os.environ.get("TRT_ENGINES_CACHE", "./models/engines")
    )


def civitai_cache_dir() -> str:
    # reference lib/utils.py:6-10
    return os.environ.get("CIVITAI_CACHE", "./models/civitai")


def warmup_frames() -> int:
    # reference lib/tracks.py:17 (default 10)
    return _env_int("WARMUP_FRAMES", 10)


def drop_frames() -> int:
    # reference lib/tracks.py:18 (default 0)
    return _env_int("DROP_FRAMES", 0)


def hw_encode_enabled() -> bool:
    # reference Dockerfile:54 NVENC=true; we accept both spellings
    return _env_bool("VCN_ENC", _env_bool("NVENC", False))


def hw_decode_enabled() -> bool:
    return _env_bool("VCN_DEC", _env_bool("NVDEC", False))


def media_yuv() -> bool:
    """YUV 4:2:0 end to end (default off): decoders hand out I420 frames,
    the engine converts them on the GPU and returns I420 for the encoder
    (frame format: ops/interface.py)."""
    return _env_bool("AIRTC_MEDIA_YUV", False)


def parse_lora_adapter(spec: str) -> tuple:
    """--lora-adapter NAME=PATH[:SCALE] -> (name, path, scale). The scale is
    what follows the LAST colon when that parses as a number."""
    name, eq, rest = spec.partition("=")
    if not eq or not name or not rest:
        raise ValueError(f"a LoRA adapter is NAME=PATH[:SCALE], got {spec!r}")
    path, colon, tail = rest.rpartition(":")
    scale = 1.0
    if colon:
        try:
            scale = float(tail)
        except ValueError:
            path = rest
    else:
        path = rest
    if not path or not math.isfinite(scale):
        raise ValueError(f"a LoRA adapter is NAME=PATH[:SCALE], got {spec!r}")
    return name, path, scale


def lora_adapter_specs(specs=None) -> list:
    """The adapters to load at start-up: the given NAME=PATH[:SCALE] strings,
    else $AIRTC_LORA_ADAPTER_FILES (comma-separated), parsed; names unique."""
    if specs is None:
        env = os.environ.get("AIRTC_LORA_ADAPTER_FILES", "")
        specs = [s for s in env.split(",") if s.strip()]
    out = [parse_lora_adapter(s.strip()) for s in specs]
    names = [n for n, _, _ in out]
    if len(set(names)) != len(names):
        raise ValueError(f"LoRA adapter names must be unique, got {names}")
    return out


OUTPUT_FORMATS = ("rgb", "i420")
OUTPUT_SIZES = ("engine", "source")
CONTROLNET_PROCESSORS = ("none", "canny")
SAFETY_CHECKERS = ("tiny", "clip")


@dataclass
class EncoderConfig:
    """VCN encoder knobs — parity with reference NVENC_* env surface."""

    preset: str = field(default_factory=lambda: os.environ.get("VCN_ENC_PRESET", os.environ.get("NVENC_PRESET", "P3")))
    tuning_info: str = field(default_factory=lambda: os.environ.get("VCN_ENC_TUNING_INFO", os.environ.get("NVENC_TUNING_INFO", "low_latency")))
    default_bitrate: int = field(default_factory=lambda: _env_int("VCN_ENC_DEFAULT_BITRATE", _env_int("NVENC_DEFAULT_BITRATE", 4_000_000)))
    min_bitrate: int = field(default_factory=lambda: _env_int("VCN_ENC_MIN_BITRATE", _env_int("NVENC_MIN_BITRATE", 1_000_000)))
    max_bitrate: int = field(default_factory=lambda: _env_int("VCN_ENC_MAX_BITRATE", _env_int("NVENC_MAX_BITRATE", 8_000_000)))


@dataclass
class SimilarityFilterConfig:
    """Stochastic similarity filter (reference lib/wrapper.py:57-59,192-195)."""

    enabled: bool = False
    threshold: float = 0.98
    max_skip_frame: int = 10


@dataclass
class EngineConfig:
    """Full pipeline configuration.

    Defaults reproduce the reference's production config
    (reference lib/pipeline.py:11-14,23-36; lib/wrapper.py:46-65).
    """

    model_id: str = "lykon/dreamshaper-8"
    model_family: str = "sd15"  # sd15 | sd21 (sd-turbo) | sdxl
    width: int = 512
    height: int = 512
    t_index_list: List[int] = field(default_factory=lambda: [18, 26, 35, 45])
    num_inference_steps: int = 50
    guidance_scale: float = 0.0
    cfg_type: str = "self"  # none | full | self | initialize
    delta: float = 1.0
    frame_buffer_size: int = 1
    use_denoising_batch: bool = True
    use_lcm_lora: bool = True
    # False: the checkpoint's own AutoencoderKL (models/vae_kl.py) instead of
    # TAESD, as the reference's use_tiny_vae=False. Not for sdxl (below).
    use_tiny_vae: bool = field(default_factory=lambda: _env_bool("AIRTC_TINY_VAE", True))
    do_add_noise: bool = True
    dtype: str = "float16"
    seed: int = 2
    mode: str = "img2img"  # img2img | txt2img
    prompt: str = "fireworks in the night sky"  # reference lib/pipeline.py:11
    negative_prompt: str = ""
    lora_dict: Optional[dict] = None
    lcm_lora_id: Optional[str] = None
    vae_id: Optional[str] = None
    use_controlnet: bool = False
    controlnet_scale: float = field(default_factory=lambda: _env_float("AIRTC_CONTROLNET_SCALE", 1.0))
    use_safety_checker: bool = False
    # which checker use_safety_checker builds: "tiny" = the small conv
    # classifier (models/safety.py), "clip" = the reference's
    # StableDiffusionSafetyChecker (models/safety_clip.py: CLIP ViT-L/14
    # image tower, cosine against concept embeddings), run inside the
    # captured decode graph. safety_adjustment is that checker's
    # `adjustment`, added to every score (positive is stricter); per serving
    # slot at run time through engine.update_safety, which is deliberately
    # not reachable from POST /config or the datachannel.
    safety_checker: str = field(default_factory=lambda: os.environ.get("AIRTC_SAFETY_CHECKER") or "tiny")
    safety_adjustment: float = field(default_factory=lambda: _env_float("AIRTC_SAFETY_ADJUSTMENT", 0.0))
    similarity_filter: SimilarityFilterConfig = field(default_factory=SimilarityFilterConfig)
    encoder: EncoderConfig = field(default_factory=EncoderConfig)
    device: str = "cuda"
    # engine acceleration: "hip" (hand-written kernels + hipGraph) or "eager"
    acceleration: str = "hip"
    use_hip_graph: bool = True
    # overlap VAE-decode+postprocess of frame i with frame i+1's denoise on a
    # second HIP stream (pipelined graphs; disabled automatically when the
    # similarity filter needs a per-frame decision)
    pipeline_overlap: bool = True
    # fp8 (OCP e4m3) serving tier: the resnet GN->conv pairs quantize
    # producer-side (GN writes e4m3 codes, conv runs on the MX-scaled MFMA
    # at 2x the f16 rate with half the activation traffic). Per-layer
    # activation scales calibrate on the first fp8_calib_frames real frames,
    # then a UNet-forward quality gate must pass fp8_min_snr_db or the
    # engine falls back to f16. fp16 stays the benchmarked default
    # (MI355X-native addition; no reference counterpart).
    use_fp8: bool = field(default_factory=lambda: _env_bool("AIRTC_FP8", False))
    fp8_calib_frames: int = field(default_factory=lambda: _env_int("AIRTC_FP8_CALIB_FRAMES", 8))
    fp8_margin: float = field(default_factory=lambda: _env_float("AIRTC_FP8_MARGIN", 1.5))
    fp8_min_snr_db: float = field(default_factory=lambda: _env_float("AIRTC_FP8_MIN_SNR_DB", 16.0))

    # any-resolution ingest: how a frame whose size is not (height, width)
    # is fitted into the engine's input slot on the device
    # (ops.fit_frame_u8): cover = centred crop to the engine aspect, then
    # resize; contain = whole frame with black bars; stretch = whole frame,
    # aspect not kept. Engine-sized frames are never touched.
    fit_mode: str = field(default_factory=lambda: os.environ.get("AIRTC_FIT_MODE") or "cover")

    # what the engine returns: "rgb" = (H,W,3) u8 as ever, "i420" = (3H/2,W)
    # u8 planes ready for the codec (needs even height and width). Input
    # frames may be either format whatever this says.
    output_format: str = field(default_factory=lambda: "i420" if media_yuv() else "rgb")

    # any-resolution egress: "engine" = every frame comes back at (height,
    # width), as ever; "source" = each slot's frame is resized back on the
    # device to the size its session published (ops.unfit_geometry: contain
    # loses its bars, cover returns the part of the source that was used),
    # so a call returns one tensor per slot and their sizes may differ.
    # output_max_side > 0 caps the longer side of a returned frame: the
    # software encoder's cost grows with the outgoing pixel count.
    output_size: str = field(default_factory=lambda: os.environ.get("AIRTC_OUTPUT_SIZE") or "engine")
    output_max_side: int = field(default_factory=lambda: _env_int("AIRTC_OUTPUT_MAX_SIDE", 0))

    # keep the RCFG step (and for cfg full/initialize its extra UNet rows) in
    # the captured graph whatever the initial guidance_scale, so that
    # update_guidance() can raise guidance later, per serving slot, without
    # a re-capture. Off: an engine prepared with guidance_scale <= 1 has no
    # guidance math in its hot path at all (the benchmarked graphs).
    runtime_guidance: bool = field(default_factory=lambda: _env_bool("AIRTC_RUNTIME_GUIDANCE", False))

    # ControlNet conditioning processor (use_controlnet, img2img): "none"
    # hands the ControlNet the normalised input frame itself, the newest
    # frame's for every in-flight stage; "canny" turns each new frame into
    # the edge map an edge ControlNet was trained on (ops.canny_hint, inside
    # the captured graph), encodes it once and keeps the encoded hints of the
    # in-flight stages in a FIFO beside the latent buffer, so every stage is
    # conditioned on its own frame. canny_low/canny_high are thresholds on
    # the L1 gradient magnitude (<= 2040), per serving slot at run time
    # (update_canny); canny_reach bounds the hysteresis to that many 3x3
    # steps from a strong edge (cv2.Canny's is unbounded) and is fixed for
    # the life of the engine.
    controlnet_processor: str = field(default_factory=lambda: os.environ.get("AIRTC_CONTROLNET_PROCESSOR") or "none")
    canny_low: int = field(default_factory=lambda: _env_int("AIRTC_CANNY_LOW", 100))
    canny_high: int = field(default_factory=lambda: _env_int("AIRTC_CANNY_HIGH", 200))
    canny_reach: int = field(default_factory=lambda: _env_int("AIRTC_CANNY_REACH", 16))

    # per-session LoRA under batched serving: lora_adapters > 0 keeps that
    # many adapters unfused in a device-resident bank (models/lora.py:
    # LoraBank) and adds scale_b * (x_b A_a^T) B_a^T to every transformer
    # projection inside the captured graph (ops.lora_delta_), adapter and
    # scale read per batch row from a table engine.update_lora rewrites in
    # place. 0 (default): no bank, no launch, the graphs of before.
    # lora_max_rank bounds an adapter's rank (the bank rounds it up to 16,
    # 32 or 64). Not with use_fp8 (below).
    lora_adapters: int = field(default_factory=lambda: _env_int("AIRTC_LORA_ADAPTERS", 0))
    lora_max_rank: int = field(default_factory=lambda: _env_int("AIRTC_LORA_MAX_RANK", 32))

    def __post_init__(self) -> None:
        for name, lo, hi in (("lora_adapters", 0, 64), ("lora_max_rank", 1, 64)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an int, got {v!r}")
            if not lo <= v <= hi:
                raise ValueError(f"{name} must be in [{lo}, {hi}], got {v}")
        if self.lora_adapters > 0 and self.use_fp8:
            raise ValueError(
                "lora_adapters > 0 is not available with use_fp8: the fp8 "
                "tier's activation scales are calibrated once, and nobody has "
                "measured them against a per-slot weight change")
        if not self.use_tiny_vae and self.model_family in ("sdxl", "tiny_xl"):
            raise ValueError(
                f"use_tiny_vae=False is not available for model_family="
                f"{self.model_family!r}: SDXL's AutoencoderKL overflows "
                f"float16, and its float32-upcast route is not built; keep "
                f"the tiny VAE for sdxl")
        if self.safety_checker not in SAFETY_CHECKERS:
            raise ValueError(
                f"safety_checker must be one of {SAFETY_CHECKERS}, "
                f"got {self.safety_checker!r}")
        if isinstance(self.safety_adjustment, bool) \
                or not isinstance(self.safety_adjustment, (int, float)) \
                or not math.isfinite(self.safety_adjustment):
            raise ValueError(
                f"safety_adjustment must be a finite number, got "
                f"{self.safety_adjustment!r}")
        if self.controlnet_processor not in CONTROLNET_PROCESSORS:
            raise ValueError(
                f"controlnet_processor must be one of {CONTROLNET_PROCESSORS}, "
                f"got {self.controlnet_processor!r}")
        for name in ("canny_low", "canny_high", "canny_reach"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an int, got {v!r}")
        if not 0 <= self.canny_low <= self.canny_high <= 2040:
            raise ValueError(
                f"canny thresholds need 0 <= canny_low <= canny_high <= 2040, "
                f"got {self.canny_low}, {self.canny_high}")
        if not 0 <= self.canny_reach <= 32:
            raise ValueError(
                f"canny_reach must be in [0, 32], got {self.canny_reach}")
        if self.output_format not in OUTPUT_FORMATS:
            raise ValueError(
                f"output_format must be one of {OUTPUT_FORMATS}, got {self.output_format!r}")
        if self.output_size not in OUTPUT_SIZES:
            raise ValueError(
                f"output_size must be one of {OUTPUT_SIZES}, got {self.output_size!r}")
        if not isinstance(self.output_max_side, int) or self.output_max_side < 0:
            raise ValueError(
                f"output_max_side must be an int >= 0, got {self.output_max_side!r}")

    @property
    def denoising_steps(self) -> int:
        return len(self.t_index_list)

    @property
    def unet_batch(self) -> int:
        """The stream-batch law (reference lib/wrapper.py:159-163)."""
        if self.use_denoising_batch:
            b = self.denoising_steps * self.frame_buffer_size
            if self.cfg_type == "initialize":
                b += self.frame_buffer_size
            elif self.cfg_type == "full":
                b *= 2
            return b
        return self.frame_buffer_size

    @property
    def latent_height(self) -> int:
        return self.height // 8

    @property
    def latent_width(self) -> int:
        return self.width // 8


def sd_turbo_config(**kw) -> EngineConfig:
    """BASELINE.json headline config: SD-Turbo 512x512 1-step img2img."""
    defaults = dict(
        model_id="stabilityai/sd-turbo",
        model_family="sd21",
        t_index_list=[0],
        num_inference_steps=1,
        guidance_scale=0.0,
        cfg_type="none",
        use_lcm_lora=False,
        use_tiny_vae=True,
    )
    defaults.update(kw)
    return EngineConfig(**defaults)
