"""StreamDiffusionEngine — the per-frame diffusion engine.

From-scratch replacement for reference L4+L5 (lib/wrapper.py +
the external StreamDiffusion package). Public surface mirrors the
reference wrapper contract:

- ctor option surface            (reference lib/wrapper.py:34-132)
- prepare(prompt, steps, g)      (reference lib/wrapper.py:197-234)
- __call__/img2img/txt2img       (reference lib/wrapper.py:236-343)
- update_prompt                  (reference lib/pipeline.py:44-45)
- update_t_index_list            (reference lib/wrapper.py:389-407)
- stream-batch law B = len(t_index)*frame_buffer (lib/wrapper.py:159-163)

MI355X-native execution: the whole per-frame step (VAE encode -> stream-batch
UNet -> scheduler -> VAE decode) runs over static device buffers so it can be
captured ONCE into a hipGraph (torch.cuda.CUDAGraph is hipGraph on ROCm) and
replayed per frame — this replaces the reference's TensorRT engine loading
(lib/wrapper.py:409-512). Prompt and t_index updates write into
graph-external buffers in place; the graph is never re-captured
(SURVEY.md §7 hard part #2).
"""
from __future__ import annotations

from typing import Optional, Sequence

import contextlib
import dataclasses
import logging
import math
import os

import torch

from ..config import EngineConfig
from ..models import TinyVAE, TextEncoder, UNet2DCondition, UNetConfig
from ..models.lora import fuse_lora_state_dict, load_lora_file, make_random_lora
from ..utils.timers import StageTimers
from .. import ops
from .rcfg import ResidualCFG
from .scheduler import StreamScheduler, slot_rows
from .similarity import StochasticSimilarityFilter


def _unet_config_for(family: str) -> UNetConfig:
    return {
        "sd15": UNetConfig.sd15,
        "sd21": UNetConfig.sd21,
        "sdxl": UNetConfig.sdxl,
        "tiny": UNetConfig.tiny,
        "tiny_xl": UNetConfig.tiny_xl,
    }[family]()


# update_lora(adapter=LORA_KEEP, scale=...): the scale alone, adapter as it is
LORA_KEEP = object()


class StreamDiffusionEngine:
    def __init__(
        self,
        cfg: EngineConfig,
        unet: Optional[UNet2DCondition] = None,
        vae: Optional[TinyVAE] = None,
        text_encoder: Optional[TextEncoder] = None,
        safety_checker: Optional[torch.nn.Module] = None,
    ) -> None:
        self.cfg = cfg
        # per-session adapter bank, built by prepare() when cfg.lora_adapters > 0
        self._lora_bank = None
        if cfg.output_format not in ("rgb", "i420"):
            raise ValueError(
                f"output_format must be 'rgb' or 'i420', got {cfg.output_format!r}")
        if cfg.output_format == "i420" and (cfg.height % 2 or cfg.width % 2):
            raise ValueError(
                f"output_format='i420' needs even height and width, got "
                f"{cfg.height}x{cfg.width}")
        self.device = torch.device(cfg.device if torch.cuda.is_available() or cfg.device == "cpu" else "cpu")
        self.dtype = getattr(torch, cfg.dtype) if self.device.type == "cuda" else torch.float32
        torch.manual_seed(cfg.seed)

        self.scheduler = StreamScheduler(num_inference_steps=cfg.num_inference_steps)
        self.rcfg = ResidualCFG(cfg.cfg_type, cfg.guidance_scale, cfg.delta,
                                runtime=cfg.runtime_guidance)
        self.sim_filter: Optional[StochasticSimilarityFilter] = None
        if cfg.similarity_filter.enabled:
            gen = torch.Generator().manual_seed(cfg.seed)
            self.sim_filter = StochasticSimilarityFilter(
                cfg.similarity_filter.threshold, cfg.similarity_filter.max_skip_frame, gen
            )

        ucfg = _unet_config_for(cfg.model_family)
        self.unet = unet if unet is not None else UNet2DCondition(ucfg)
        if vae is not None:
            self.vae = vae
        elif cfg.use_tiny_vae:
            self.vae = TinyVAE()
        else:
            # the checkpoint's full AutoencoderKL; the tiny test family gets
            # a two-block stand-in of the same architecture
            from ..models.vae_kl import (AutoencoderKLVAE, KLConfig,
                                         TINY_KL_CONFIG)
            self.vae = AutoencoderKLVAE(
                TINY_KL_CONFIG if cfg.model_family == "tiny" else KLConfig(),
                device=self.device)
        # family conventions: SD1.5 = CLIP ViT-L/14 (quick-gelu, last
        # layer); SD2.x = OpenCLIP ViT-H (gelu, PENULTIMATE layer, 23
        # blocks); sdxl = the DUAL encoder (ViT-L + OpenCLIP bigG, both
        # penultimate, per-token concat to 2048, pooled from bigG)
        if text_encoder is not None:
            self.text_encoder = text_encoder
        elif ucfg.addition_embed_dim:
            from ..models.text_encoder import DualTextEncoder

            if cfg.model_family == "sdxl":
                self.text_encoder = DualTextEncoder()
            else:  # tiny_xl: small dual with the same contract
                half = ucfg.cross_attention_dim // 2
                self.text_encoder = DualTextEncoder(
                    hidden1=half, layers1=2,
                    hidden2=ucfg.cross_attention_dim - half, layers2=2,
                    vocab_size=512)
        else:
            if cfg.model_family == "tiny":
                te_layers, te_act, te_skip = 2, "quick_gelu", 0
            elif cfg.model_family == "sd21":
                te_layers, te_act, te_skip = 23, "gelu", 1
            else:
                te_layers, te_act, te_skip = 12, "quick_gelu", 0
            self.text_encoder = TextEncoder(
                hidden=ucfg.cross_attention_dim,
                layers=te_layers,
                act=te_act,
                clip_skip=te_skip,
            )
        self.ctx_dim = ucfg.cross_attention_dim
        self.addition_embed_dim = ucfg.addition_embed_dim

        self.controlnet = None
        if cfg.use_controlnet:
            from ..models.controlnet import ControlNet

            self.controlnet = ControlNet(ucfg)
        self.safety_checker = None
        # safety_checker="clip": the reference's CLIP checker, decided and
        # applied on the device inside the decode graph (_decode_core)
        self._clip_safety = False
        if cfg.use_safety_checker and cfg.safety_checker == "clip":
            from ..models.safety_clip import ClipSafetyChecker

            self.safety_checker = (safety_checker if safety_checker is not None
                                   else ClipSafetyChecker())
            self._clip_safety = True
        elif cfg.use_safety_checker:
            from ..models.safety import SafetyChecker

            self.safety_checker = SafetyChecker()

        # real weights when available: model_id as a local diffusers-style
        # dir, or an HF-cache snapshot (random init otherwise — offline)
        self._load_weights_if_present(cfg.model_id)
        if self._clip_safety:
            from ..models.load import load_safety_checker_if_present

            # the checker's own repository in the HF cache, when the model
            # directory brought none
            load_safety_checker_if_present(self.safety_checker)
            if self.safety_checker.weights != "loaded":
                logging.getLogger(__name__).warning(
                    "safety checker: no checkpoint found, the CLIP checker "
                    "runs on random weights and its verdicts mean nothing")

        # LoRA fusion happens BEFORE device placement / graph capture
        # (reference fuses before TRT compile, lib/wrapper.py:645-697).
        if cfg.use_lcm_lora:
            sd = (
                load_lora_file(cfg.lcm_lora_id)
                if cfg.lcm_lora_id
                else make_random_lora(self.unet, rank=4, seed=cfg.seed)
            )
            fuse_lora_state_dict(self.unet, sd, scale=1.0)
        if cfg.lora_dict:
            for path, scale in cfg.lora_dict.items():
                fuse_lora_state_dict(self.unet, load_lora_file(path), scale=scale)

        self.unet = self.unet.to(self.device, self.dtype).eval()
        self.vae = self.vae.to(self.device, self.dtype).eval()
        self.text_encoder = self.text_encoder.to(self.device).eval()
        if self.controlnet is not None:
            self.controlnet = self.controlnet.to(self.device, self.dtype).eval()
        if self.safety_checker is not None:
            self.safety_checker = self.safety_checker.to(self.device, self.dtype).eval()

        self.timers = StageTimers(use_cuda=self.device.type == "cuda")
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._prepared = False
        self.prompt: str = cfg.prompt

        # fp8 serving tier (opt-in): calibrate per-layer activation scales
        # on the first real frames (eager), freeze + quality-gate, then the
        # graph captures the GN-fp8 -> MX-MFMA conv path. fp16 stays the
        # default; incompatible with the env-gated AIRTC_FUSE_GN experiment
        # (that path bypasses the GN apply kernel entirely).
        self._fp8_norms: list = []
        self._fp8_calib_left = 0
        self.fp8_active = False
        self.fp8_snr_db: Optional[float] = None
        self._fp8_vae: dict = {"convs": [], "outs": []}
        if cfg.use_fp8 and os.environ.get("AIRTC_FUSE_GN") != "1":
            from ..models.taesd import fp8_flag_convs
            from ..models.unet import fp8_eligible_norms

            self._fp8_norms = fp8_eligible_norms(self.unet)
            if self.controlnet is not None:
                # ControlNet shares the resnet blocks — same tier applies
                self._fp8_norms += fp8_eligible_norms(self.controlnet)
            for nrm in self._fp8_norms:
                nrm._fp8_calibrate = True
                nrm._fp8_amax = 0.0
            if cfg.use_tiny_vae:
                self._fp8_vae = fp8_flag_convs(self.vae)
                for c in self._fp8_vae["convs"]:
                    c._fp8_calibrate = True
                    c._fp8_in_amax = 0.0
                    c._fp8_out_amax = 0.0
            self._fp8_calib_left = max(1, cfg.fp8_calib_frames)

    def _load_weights_if_present(self, model_id: str) -> None:
        import glob
        import os

        from ..models.load import load_model_dir

        candidates = [model_id] if os.path.isdir(model_id) else []
        hub = os.environ.get("HF_HUB_CACHE", os.path.expanduser("~/.cache/huggingface/hub"))
        candidates += glob.glob(
            os.path.join(hub, "models--" + model_id.replace("/", "--"), "snapshots", "*")
        )
        for c in candidates:
            try:
                if load_model_dir(self, c):
                    return
            except Exception:  # corrupt cache entry: keep random init
                continue

    # ------------------------------------------------------------------
    # prepare
    # ------------------------------------------------------------------
    @torch.no_grad()
    def prepare(
        self,
        prompt: Optional[str] = None,
        num_inference_steps: Optional[int] = None,
        guidance_scale: Optional[float] = None,
        t_index_list: Optional[Sequence[int]] = None,
    ) -> None:
        cfg = self.cfg
        if prompt is not None:
            self.prompt = prompt
        if num_inference_steps is not None:
            cfg.num_inference_steps = num_inference_steps
            self.scheduler = StreamScheduler(num_inference_steps=num_inference_steps)
        if guidance_scale is not None:
            cfg.guidance_scale = guidance_scale
            self.rcfg = ResidualCFG(cfg.cfg_type, guidance_scale, cfg.delta,
                                    runtime=cfg.runtime_guidance)
        if t_index_list is not None:
            cfg.t_index_list = list(t_index_list)

        n = cfg.denoising_steps
        fbs = cfg.frame_buffer_size
        B = n * fbs
        lh, lw = cfg.latent_height, cfg.latent_width
        dev, dt = self.device, self.dtype

        # coefficients live in the engine compute dtype: scheduler tensor math
        # must not promote the latent out of f16 (the HIP dispatch dtype)
        self._coeff = self.scheduler.coefficients(cfg.t_index_list, fbs, dev, self.dtype)
        # NHWC coefficient views: (B,1,1,1) already broadcast over (B,h,w,c)
        self._embeds = self.text_encoder.encode(self.prompt, dev, dt)
        self._embeds_batch = self._embeds.expand(B, -1, -1).contiguous()
        if cfg.cfg_type == "full":
            neg = self.text_encoder.encode(cfg.negative_prompt, dev, dt)
            self._embeds_full = torch.cat([neg.expand(B, -1, -1), self._embeds_batch], dim=0).contiguous()

        # sdxl addition conditioning: pooled text (1280) + 6 sinusoidal
        # time-id embeddings of 256 (orig h/w, crop t/l, target h/w) = 2816
        self._added_cond = None
        if self.addition_embed_dim:
            self._added_cond = torch.zeros((B, self.addition_embed_dim), device=dev, dtype=dt)
            self._refresh_added_cond()

        g = torch.Generator(device="cpu").manual_seed(cfg.seed)
        self._init_noise = torch.randn((B, lh, lw, 4), generator=g).to(dev, dt)
        self._x_t_buffer = torch.zeros((max(0, B - fbs), lh, lw, 4), device=dev, dtype=dt)
        # controlnet_processor == "canny": the encoded edge hints of the
        # in-flight stages, row for row beside _x_t_buffer (stage i+1 of
        # the next round reads what stage i read in this one), and the
        # per-slot (low, high) thresholds the kernel reads from memory
        self._canny = (cfg.controlnet_processor == "canny"
                       and self.controlnet is not None and cfg.mode == "img2img")
        self._hint_feat_buffer = None
        self._canny_thr = None
        if self._canny:
            c0 = self.controlnet.cfg.block_out_channels[0]
            self._hint_feat_buffer = torch.zeros((max(0, B - fbs), lh, lw, c0), device=dev, dtype=dt)
            self._canny_thr = torch.tensor(
                [[cfg.canny_low, cfg.canny_high]] * fbs, dtype=torch.int32).to(dev)
        self.rcfg.reset(self._init_noise)
        # clip safety checker: the per-slot adjustment the head kernel reads
        # from memory and the per-slot count of flagged frames it keeps
        # (read back only by stats()); the counts outlive a re-prepare
        self._safety_adjust = None
        if self._clip_safety:
            self._safety_adjust = torch.full(
                (fbs,), float(cfg.safety_adjustment), dtype=torch.float32).to(dev)
            cnt = getattr(self, "_safety_count", None)
            if cnt is None or cnt.shape[0] != fbs:
                self._safety_count = torch.zeros(fbs, dtype=torch.int32, device=dev)

        # static I/O buffers (graph-stable addresses); _frame_in (u8) is the
        # only per-frame input — preprocess lives inside the graph
        self._frame_in = torch.zeros((fbs, cfg.height, cfg.width, 3), device=dev, dtype=torch.uint8)
        if cfg.fit_mode not in ops.FIT_MODES:
            raise ValueError(f"fit_mode must be one of {ops.FIT_MODES}, got {cfg.fit_mode!r}")
        # last source (height, width) seen per slot — stats()["ingest"]
        self._src_size: list = [None] * fbs
        # "rgb" / "i420" as last handed in per slot
        self._src_format: list = [None] * fbs
        # per-slot runtime controls, host side (slot_controls()/stats): every
        # slot starts from the replica defaults
        self._slot_ctl: list = [self._slot_defaults() for _ in range(fbs)]
        self._ts_batch = self._coeff["sub_timesteps_tensor"].to(dev)
        self._prev_out: Optional[torch.Tensor] = None
        # any-resolution egress (cfg.output_size == "source"): per-slot
        # [Ht, Wt] of the frames last returned (stats) and of the call that
        # produced _prev_out (the similarity filter never answers a session
        # with a frame of another size)
        self._egress = cfg.output_size == "source"
        self._out_size: list = [None] * fbs
        self._prev_sizes: Optional[list] = None
        self._graph = None
        self._pipelined = False
        self._last_done = None
        self._prepared = True
        self._prepare_lora()
        self._refresh_static_kv()
        self._ts_unet_cache = None
        self._refresh_temb_static()

    def _cross_attn_modules(self):
        from ..models.unet import CrossAttention

        mods = []
        for root in (self.unet, self.controlnet):
            if root is None:
                continue
            for name, m in root.named_modules():
                if isinstance(m, CrossAttention) and name.endswith("attn2"):
                    mods.append(m)
        return mods

    @torch.no_grad()
    def _refresh_static_kv(self) -> None:
        """Precompute every cross-attention layer's K|V from the (static)
        text embeddings. K/V depend only on the prompt, so these GEMMs run
        at prepare()/update_prompt() instead of once per frame; the hot
        graph reads the static buffers (stable addresses, copy_ on update)."""
        ctx = self._unet_batch_embeds()
        for m in self._cross_attn_modules():
            kv = m.compute_kv(ctx)
            cur = getattr(m, "static_kv", None)
            if cur is None or cur.shape != kv.shape or cur.dtype != kv.dtype:
                m.static_kv = kv.contiguous()
            else:
                cur.copy_(kv)

    @torch.no_grad()
    def _added_cond_vec(self, prompt: str) -> torch.Tensor:
        """The sdxl addition-embedding (1, addition_embed_dim) of a prompt."""
        from ..models.unet import timestep_embedding

        cfg = self.cfg
        pooled = self.text_encoder.pooled(prompt, self.device, self.dtype)
        ids = torch.tensor(
            [cfg.height, cfg.width, 0, 0, cfg.height, cfg.width],
            dtype=torch.float32, device=self.device,
        )
        time_emb = timestep_embedding(ids, 256).flatten()[None].to(self.dtype)
        return torch.cat([pooled, time_emb], dim=-1)

    @torch.no_grad()
    def _refresh_added_cond(self) -> None:
        """(Re)compute the sdxl addition-embedding into its static buffer."""
        vec = self._added_cond_vec(self.prompt)
        self._added_cond.copy_(vec.expand_as(self._added_cond))

    # ------------------------------------------------------------------
    # weight hot-swap (LoRA) — SURVEY.md §5.8 / N12: fuse, invalidate the
    # kernel-side weight caches, re-broadcast over RCCL when distributed,
    # and drop the hipGraphs (re-captured on the next frame)
    # ------------------------------------------------------------------
    @torch.no_grad()
    def load_lora(self, path_or_sd, scale: float = 1.0) -> int:
        sd = load_lora_file(path_or_sd) if isinstance(path_or_sd, str) else path_or_sd
        n = fuse_lora_state_dict(self.unet, sd, scale=scale)
        self.refresh_weights()
        return n

    @torch.no_grad()
    def refresh_weights(self) -> None:
        """After any in-place weight change: drop the lazily-built GPU weight
        transforms (conv GEMM layouts, fused QKV, f32 bias copies), re-sync
        replicas, and force a graph re-capture."""
        for module in (self.unet, self.vae, self.controlnet,
                       self.safety_checker if self._clip_safety else None):
            if module is not None:
                ops.drop_weight_caches(module)
        from ..parallel.collectives import broadcast_engine_weights

        broadcast_engine_weights(self)  # no-op at world_size 1
        if self._prepared:
            self._refresh_static_kv()
            self._refresh_temb_static()  # time-emb MLP weights changed
        # fp8 tier: new weights shift the activation distributions — drop
        # back to calibration (a few eager frames) and re-gate
        if self.cfg.use_fp8 and (self._fp8_norms or self._fp8_vae["convs"]):
            for nrm in self._fp8_norms:
                nrm._fp8_calibrate = True
                nrm._fp8_scale = None
                nrm._fp8_amax = 0.0
            for c in self._fp8_vae["convs"]:
                c._fp8_calibrate = True
                c._fp8_in_scale = c._fp8_out_scale = None
                c._fp8_in_amax = c._fp8_out_amax = 0.0
            self.fp8_active = False
            self._fp8_calib_left = max(1, self.cfg.fp8_calib_frames)
        if self.device.type == "cuda":
            # quiesce in-flight replays before their graphs are dropped
            torch.cuda.synchronize()
        self._graph = None  # re-capture lazily with the new weights

    # ------------------------------------------------------------------
    # per-session LoRA (cfg.lora_adapters > 0): an unfused adapter bank the
    # captured graph reads through a per-row (adapter, scale) table. Loading
    # a file into a bank index and pointing a slot at an index are in-place
    # writes: no re-capture, no refresh_weights, no device-wide synchronise.
    # The global load_lora path above is separate and unchanged.
    # ------------------------------------------------------------------
    def _prepare_lora(self) -> None:
        cfg = self.cfg
        if cfg.lora_adapters <= 0:
            return
        if self._lora_bank is None:
            from ..models.lora import LoraBank

            self._lora_bank = LoraBank(self.unet, cfg.lora_adapters,
                                       cfg.lora_max_rank)
            self._lora_names: dict = {}   # name -> bank index
            self._lora_loads: dict = {}   # name -> times loaded
            self._lora_default = (None, 1.0)
            # _slot_ctl was filled before the bank existed
            for c in self._slot_ctl:
                c["lora"], c["lora_scale"] = self._lora_default
        # the largest UNet batch of any layout: full doubles the rows,
        # initialize adds fbs; every layout keeps row % fbs == slot, so one
        # table serves them all by its prefix
        rows = 2 * cfg.denoising_steps * cfg.frame_buffer_size
        ra, rs = self._lora_bank.rows
        if ra.shape[0] != rows:
            self._lora_bank.set_rows(
                torch.full((rows,), -1, dtype=torch.int32, device=self.device),
                torch.ones(rows, dtype=torch.float32, device=self.device))
        self._write_lora_rows(refresh_kv=False)

    def _lora_name_of(self, index):
        for n, i in self._lora_names.items():
            if i == index:
                return n
        return None

    def _write_lora_rows(self, slot: Optional[int] = None,
                         refresh_kv: bool = True) -> None:
        """The (adapter, scale) of one slot (None: of every slot) into its
        rows of the tables, and with them its static cross-attention K|V,
        which carry the to_k / to_v deltas. Scalar fills: nothing is
        uploaded, and no other slot's rows are touched."""
        fbs = self.cfg.frame_buffer_size
        ra, rs = self._lora_bank.rows
        with self._row_writes():
            for s in (range(fbs) if slot is None else [slot]):
                c = self._slot_ctl[s]
                slot_rows(ra, s, fbs).fill_(-1 if c["lora"] is None else c["lora"])
                slot_rows(rs, s, fbs).fill_(c["lora_scale"])
            if not refresh_kv:
                return
            if slot is None:
                self._refresh_static_kv()
                return
            # row `slot` of the embeddings is one of the slot's rows
            self._write_slot_kv(self._embeds_batch[slot:slot + 1], slot)
            if self._layout() == "full":
                self._write_slot_kv(self._embeds_full[slot:slot + 1], slot,
                                    uncond=True)

    def _resolve_adapter(self, adapter):
        """None, a bank index or a loaded name -> None or a loaded index."""
        bank = self._lora_bank
        if adapter is None:
            return None
        if isinstance(adapter, str):
            if adapter not in self._lora_names:
                raise ValueError(
                    f"unknown LoRA {adapter!r}; loaded: {sorted(self._lora_names)}")
            return self._lora_names[adapter]
        if isinstance(adapter, bool) or not isinstance(adapter, int) \
                or not 0 <= adapter < bank.n_adapters:
            raise ValueError(
                f"adapter must be None, a loaded name or a bank index in "
                f"[0, {bank.n_adapters}), got {adapter!r}")
        if not bank.loaded[adapter]:
            raise ValueError(f"bank index {adapter} holds no adapter")
        return adapter

    def _require_bank(self):
        if self._lora_bank is None:
            raise ValueError(
                "per-session LoRA is off: build the engine with "
                "lora_adapters > 0 (AIRTC_LORA_ADAPTERS)")
        return self._lora_bank

    @torch.no_grad()
    def load_adapter(self, index: int, path_or_sd, scale: float = 1.0,
                     name: Optional[str] = None) -> dict:
        """Load an adapter file (kohya, diffusers/PEFT or own-path keys) into
        bank index `index`, in place, under the name `name`. Slots that point
        at the index show the new adapter from the next frame. Returns the
        loader's counts (LoraBank.load).

        Like every update_* call it must come from the thread that calls the
        engine, never concurrently with __call__: the bank is rewritten by
        one copy per target on the denoise stream, and a replay enqueued
        between two of them would read an adapter half old, half new."""
        assert self._prepared, "call prepare() first"
        bank = self._require_bank()
        if name is not None and (not isinstance(name, str) or not name):
            raise ValueError(f"name must be a non-empty string, got {name!r}")
        if name is not None and self._lora_names.get(name, index) != index:
            raise ValueError(
                f"LoRA name {name!r} already names bank index "
                f"{self._lora_names[name]}")
        sd = load_lora_file(path_or_sd) if isinstance(path_or_sd, str) else path_or_sd
        used = any(c["lora"] == index for c in self._slot_ctl)
        counts = bank.load(index, sd, scale=scale, ordered=self._row_writes,
                           after=self._refresh_static_kv if used else None)
        for n in [n for n, i in self._lora_names.items() if i == index]:
            del self._lora_names[n]
        if name is not None:
            self._lora_names[name] = index
            self._lora_loads[name] = self._lora_loads.get(name, 0) + 1
        return counts

    @torch.no_grad()
    def update_lora(self, adapter=None, scale: Optional[float] = None,
                    slot: Optional[int] = None) -> None:
        """Point a slot (slot=None: every slot, and the default reset_slot()
        restores) at an adapter: a bank index, a loaded name, None for no
        adapter, or LORA_KEEP to change the scale alone. scale=None keeps
        the slot's scale. Everything is validated before the first write."""
        self._check_slot(slot)
        self._require_bank()
        keep = adapter is LORA_KEEP
        index = None if keep else self._resolve_adapter(adapter)
        if scale is not None:
            if isinstance(scale, bool) or not isinstance(scale, (int, float)) \
                    or not math.isfinite(scale):
                raise ValueError(f"lora scale must be a finite number, got {scale!r}")
            scale = float(scale)
        for s in (range(self.cfg.frame_buffer_size) if slot is None else [slot]):
            c = self._slot_ctl[s]
            if not keep:
                c["lora"] = index
            if scale is not None:
                c["lora_scale"] = scale
        if slot is None:
            self._lora_default = (
                self._lora_default[0] if keep else index,
                self._lora_default[1] if scale is None else scale)
        self._write_lora_rows(slot)

    # ------------------------------------------------------------------
    # runtime config updates (POST /config + datachannel)
    #
    # Every updater takes slot=None (every slot: the replica-wide update,
    # which also moves the defaults reset_slot() restores) or one serving
    # slot, whose rows alone are rewritten (row law: scheduler.slot_rows).
    # ------------------------------------------------------------------
    def _slot_defaults(self) -> dict:
        cfg = self.cfg
        d = {
            "prompt": self.prompt,
            "negative_prompt": cfg.negative_prompt,
            "guidance_scale": float(cfg.guidance_scale),
            "delta": float(cfg.delta),
            "t_index_list": list(cfg.t_index_list),
        }
        if getattr(self, "_canny", False):
            d["canny_low"] = int(cfg.canny_low)
            d["canny_high"] = int(cfg.canny_high)
        if self._clip_safety:
            d["safety_adjustment"] = float(cfg.safety_adjustment)
        if self._lora_bank is not None:
            d["lora"], d["lora_scale"] = self._lora_default
        return d

    def _set_ctl(self, slot: Optional[int], **kw) -> None:
        for c in (self._slot_ctl if slot is None else [self._slot_ctl[slot]]):
            c.update(kw)

    def _check_slot(self, slot: Optional[int]) -> None:
        assert self._prepared, "call prepare() first"
        fbs = self.cfg.frame_buffer_size
        if slot is not None and not (isinstance(slot, int) and 0 <= slot < fbs):
            raise ValueError(f"slot must be an int in [0, {fbs}), got {slot!r}")

    def slot_controls(self, slot: int) -> dict:
        """The slot's current prompt, negative_prompt, guidance_scale, delta
        and t_index_list, and with the canny processor canny_low and
        canny_high (host-side copies; nothing is read from the GPU)."""
        self._check_slot(slot)
        c = dict(self._slot_ctl[slot])
        c["t_index_list"] = list(c["t_index_list"])
        return c

    def _layout(self) -> str:
        """UNet batch layout: "full" = [uncond x B | cond x B], "initialize"
        = [seed x fbs | B], "plain" = the B stream-batch rows."""
        if self.cfg.cfg_type in ("full", "initialize") and self.rcfg.active:
            return self.cfg.cfg_type
        return "plain"

    @contextlib.contextmanager
    def _row_writes(self, *produced: torch.Tensor):
        """Order in-place writes of graph-read buffers against the replays.
        With pipelined graphs the denoise graph replays on stream A while
        the caller's stream runs ahead, so the writes are enqueued on
        stream A after it waits for the caller's stream (which ran the text
        encoder and produced `produced`): a replay sees a row entirely old
        or entirely new. No host sync. Otherwise (eager, single graph, CPU)
        replays run on the caller's stream and program order is enough."""
        if (self.device.type == "cuda" and self._graph is not None
                and self._pipelined):
            cur = torch.cuda.current_stream()
            with torch.cuda.stream(self._sA):
                self._sA.wait_stream(cur)
                for t in produced:
                    # allocated on the caller's stream, read on stream A:
                    # without this the caller's next allocation could reuse
                    # the block before stream A (a frame behind) has read it
                    if t.is_cuda:
                        t.record_stream(self._sA)
                yield
        else:
            yield

    def _write_slot_kv(self, emb: torch.Tensor, slot: Optional[int],
                       uncond: bool = False) -> None:
        if self._lora_bank is not None and slot is None:
            # the slots' adapters may differ: one K|V per slot
            for s in range(self.cfg.frame_buffer_size):
                self._write_slot_kv(emb, s, uncond)
            return
        self._write_slot_kv_rows(emb, slot, uncond)

    def _write_slot_kv_rows(self, emb: torch.Tensor, slot: Optional[int],
                            uncond: bool) -> None:
        """K|V of ONE prompt (a 1-row GEMM per cross-attention layer) into
        the slot's rows of every static_kv. In the full layout the prompt
        owns the cond half and the negative prompt (uncond=True) the uncond
        half; in the others every row of the slot reads the prompt."""
        fbs = self.cfg.frame_buffer_size
        layout = self._layout()
        if uncond and layout != "full":
            return
        for m in self._cross_attn_modules():
            kv = m.static_kv
            if layout == "full":
                half = kv.shape[0] // 2
                kv = kv[:half] if uncond else kv[half:]
            # table row `slot` is one of the slot's rows (row % fbs == slot)
            rows = (None if self._lora_bank is None else
                    tuple(t[slot:slot + 1] for t in self._lora_bank.rows))
            slot_rows(kv, slot, fbs).copy_(m.compute_kv(emb, lora_rows=rows))

    @torch.no_grad()
    def update_prompt(self, prompt: str, slot: Optional[int] = None) -> None:
        """Re-encode the prompt and overwrite the cached embeddings IN PLACE
        (graph-external buffer update; reference lib/pipeline.py:44-45)."""
        self._check_slot(slot)
        emb = self.text_encoder.encode(prompt, self.device, self.dtype)
        if slot is not None:
            fbs = self.cfg.frame_buffer_size
            vec = (self._added_cond_vec(prompt)
                   if self._added_cond is not None else None)
            with self._row_writes(emb, *([] if vec is None else [vec])):
                slot_rows(self._embeds_batch, slot, fbs).copy_(emb)
                if self.cfg.cfg_type == "full":
                    B = self._embeds_batch.shape[0]
                    slot_rows(self._embeds_full[B:], slot, fbs).copy_(emb)
                self._write_slot_kv(emb, slot)
                if vec is not None:
                    slot_rows(self._added_cond, slot, fbs).copy_(vec)
                    # same inputs give the other rows the values they hold
                    self._refresh_temb_static()
            self._set_ctl(slot, prompt=prompt)
            return
        self.prompt = prompt
        self._set_ctl(None, prompt=prompt)
        with self._row_writes(emb):
            self._embeds.copy_(emb)
            self._embeds_batch.copy_(emb.expand_as(self._embeds_batch))
            if self.cfg.cfg_type == "full":
                B = self._embeds_batch.shape[0]
                self._embeds_full[B:].copy_(self._embeds_batch)
            if self._added_cond is not None:
                self._refresh_added_cond()
                self._refresh_temb_static()  # added-cond feeds the static temb
            self._refresh_static_kv()

    @torch.no_grad()
    def update_negative_prompt(self, prompt: str, slot: Optional[int] = None) -> None:
        """The uncond prompt of cfg_type "full": rewrite the uncond rows of
        the embeddings and their K|V in place. For every other cfg_type it
        is only stored, as prepare() only reads it for "full"."""
        self._check_slot(slot)
        if slot is None:
            self.cfg.negative_prompt = prompt
        self._set_ctl(slot, negative_prompt=prompt)
        if self.cfg.cfg_type != "full":
            return
        fbs = self.cfg.frame_buffer_size
        emb = self.text_encoder.encode(prompt, self.device, self.dtype)
        with self._row_writes(emb):
            B = self._embeds_batch.shape[0]
            slot_rows(self._embeds_full[:B], slot, fbs).copy_(emb)
            self._write_slot_kv(emb, slot, uncond=True)

    @torch.no_grad()
    def update_guidance(self, guidance_scale: Optional[float] = None,
                        delta: Optional[float] = None,
                        slot: Optional[int] = None) -> None:
        """Change guidance_scale and/or delta at runtime: an in-place write
        of the RCFG step's per-row coefficients (never a re-capture). The
        effective scale of a row is max(g, 1): g <= 1 passes its eps
        through. When RCFG is not active it is not in the captured graph:
        a replica-wide raise above 1 then re-prepares (as a length-changing
        update_t_index_list does), and a per-slot raise is an error — start
        with runtime_guidance=True to keep the step in the graph."""
        self._check_slot(slot)
        try:
            g = None if guidance_scale is None else float(guidance_scale)
            d = None if delta is None else float(delta)
        except TypeError as e:
            raise ValueError(f"guidance_scale and delta must be numbers: {e}") from e
        if any(v is not None and not math.isfinite(v) for v in (g, d)):
            raise ValueError("guidance_scale and delta must be finite")
        cfg = self.cfg
        kw = {}
        if g is not None:
            kw["guidance_scale"] = g
        if d is not None:
            kw["delta"] = d
        if not self.rcfg.active:
            if g is not None and g > 1.0 and cfg.cfg_type != "none":
                if slot is not None:
                    raise ValueError(
                        "RCFG is not in this engine's captured step (its "
                        "guidance_scale was <= 1 at prepare()), so one slot "
                        "cannot raise it: set runtime_guidance=True "
                        "(AIRTC_RUNTIME_GUIDANCE=1) to keep the step in")
                self._reprepare(guidance_scale=g, delta=d)
                return
            if slot is None:
                if g is not None:
                    cfg.guidance_scale = g
                if d is not None:
                    cfg.delta = d
                self.rcfg.set_guidance(g, d)
            self._set_ctl(slot, **kw)
            return
        with self._row_writes():
            self.rcfg.set_guidance(g, d, slot, cfg.frame_buffer_size)
        if slot is None:
            if g is not None:
                cfg.guidance_scale = g
            if d is not None:
                cfg.delta = d
        self._set_ctl(slot, **kw)

    @torch.no_grad()
    def update_canny(self, low: Optional[int] = None, high: Optional[int] = None,
                     slot: Optional[int] = None) -> None:
        """Change the Canny thresholds (0 <= low <= high <= 2040, on the L1
        gradient magnitude) of one serving slot, or of every slot and the
        replica defaults: an in-place write of the (fbs, 2) tensor the edge
        kernel reads from memory, never a re-capture. A value left None
        keeps what the slot has. The frames already in flight keep the hints
        they were encoded with; the next frame is the first to see the new
        thresholds."""
        self._check_slot(slot)
        if not self._canny:
            raise ValueError(
                "canny thresholds need controlnet_processor='canny' on an "
                "img2img engine with use_controlnet")
        fbs = self.cfg.frame_buffer_size
        slots = range(fbs) if slot is None else [slot]
        pairs = {
            s: ops.check_canny_thresholds(
                self._slot_ctl[s]["canny_low"] if low is None else low,
                self._slot_ctl[s]["canny_high"] if high is None else high)
            for s in slots
        }
        if slot is None:
            # the replica defaults (what reset_slot restores) move too and
            # must stay a valid pair themselves
            default = ops.check_canny_thresholds(
                self.cfg.canny_low if low is None else low,
                self.cfg.canny_high if high is None else high)
        rows = torch.tensor([pairs[s] for s in slots], dtype=torch.int32).to(self.device)
        with self._row_writes(rows):
            (self._canny_thr if slot is None
             else self._canny_thr[slot:slot + 1]).copy_(rows)
        for s, (lo, hi) in pairs.items():
            self._slot_ctl[s].update(canny_low=lo, canny_high=hi)
        if slot is None:
            self.cfg.canny_low, self.cfg.canny_high = default

    @torch.no_grad()
    def update_safety(self, adjustment: float, slot: Optional[int] = None) -> None:
        """Change the clip safety checker's adjustment (added to every score,
        positive is stricter) of one serving slot, or of every slot and the
        replica default: an in-place write of the (fbs,) f32 tensor the head
        kernel reads from memory, never a re-capture. Operator-only: it is
        not reachable from POST /config or the datachannel, a publisher
        must not be able to relax its own gate."""
        self._check_slot(slot)
        if not self._clip_safety:
            raise ValueError(
                "update_safety needs use_safety_checker with safety_checker='clip'")
        if isinstance(adjustment, bool) or not isinstance(adjustment, (int, float)) \
                or not math.isfinite(adjustment):
            raise ValueError(f"adjustment must be a finite number, got {adjustment!r}")
        adj = float(adjustment)
        fbs = self.cfg.frame_buffer_size
        rows = torch.full((fbs if slot is None else 1,), adj,
                          dtype=torch.float32).to(self.device)
        dst = self._safety_adjust if slot is None else self._safety_adjust[slot:slot + 1]
        if (self.device.type == "cuda" and self._graph is not None
                and self._pipelined):
            # the decode graph replays on stream B: order the write there,
            # as _row_writes does on stream A for the denoise graph's rows
            cur = torch.cuda.current_stream()
            with torch.cuda.stream(self._sB):
                self._sB.wait_stream(cur)
                rows.record_stream(self._sB)
                dst.copy_(rows)
        else:
            dst.copy_(rows)
        self._set_ctl(slot, safety_adjustment=adj)
        if slot is None:
            self.cfg.safety_adjustment = adj

    def _reprepare(self, guidance_scale: Optional[float] = None,
                   delta: Optional[float] = None,
                   t_index_list: Optional[list] = None) -> None:
        """A replica-wide update that needs prepare() again (another batch
        shape, or RCFG entering the step). prepare() reallocates
        graph-captured buffers (_coeff, _x_t_buffer, _frame_in) and drops
        the graphs, so quiesce first: in-flight pipelined replays on streams
        A/B must not read freed memory (the rule refresh_weights follows).
        The stream-batch state restarts for every slot, but the sessions
        keep their own controls: whatever a slot had moved away from the
        replica default is written again afterwards (a t_index_list of the
        old length cannot be; that slot takes the new default)."""
        saved = [dict(c) for c in self._slot_ctl]
        old = self._slot_defaults()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        if delta is not None:
            self.cfg.delta = delta
        if t_index_list is not None:
            self.cfg.t_index_list = list(t_index_list)
        self.prepare(guidance_scale=guidance_scale)
        n = len(self.cfg.t_index_list)
        for slot, c in enumerate(saved[: self.cfg.frame_buffer_size]):
            if c["prompt"] != old["prompt"]:
                self.update_prompt(c["prompt"], slot)
            if c["negative_prompt"] != old["negative_prompt"]:
                self.update_negative_prompt(c["negative_prompt"], slot)
            g = c["guidance_scale"] if c["guidance_scale"] != old["guidance_scale"] else None
            d = c["delta"] if c["delta"] != old["delta"] else None
            if g is not None or d is not None:
                self.update_guidance(g, d, slot)
            if c["t_index_list"] != old["t_index_list"] and len(c["t_index_list"]) == n:
                self.update_t_index_list(c["t_index_list"], slot)
            if self._canny and (c["canny_low"], c["canny_high"]) != (
                    old["canny_low"], old["canny_high"]):
                self.update_canny(c["canny_low"], c["canny_high"], slot)
            if self._clip_safety and c["safety_adjustment"] != old["safety_adjustment"]:
                self.update_safety(c["safety_adjustment"], slot)
            if self._lora_bank is not None and (c["lora"], c["lora_scale"]) != (
                    old["lora"], old["lora_scale"]):
                self.update_lora(adapter=c["lora"], scale=c["lora_scale"], slot=slot)

    @staticmethod
    def _tensors_of(coeff: dict) -> list:
        return [v for v in coeff.values() if isinstance(v, torch.Tensor)]

    def _update_slot_t_index_list(self, t_index_list: list, slot: int) -> None:
        cfg = self.cfg
        fbs = cfg.frame_buffer_size
        if len(t_index_list) != len(cfg.t_index_list):
            raise ValueError(
                f"a per-slot t_index_list must keep the replica's length "
                f"{len(cfg.t_index_list)}, got {len(t_index_list)}")
        new = self.scheduler.coefficients(t_index_list, fbs, self.device, self.dtype)
        new_ts = new["sub_timesteps_tensor"].to(self.device)
        with self._row_writes(new_ts, *self._tensors_of(new)):
            for k in ("alpha_prod_t_sqrt", "beta_prod_t_sqrt", "c_skip", "c_out",
                      "alpha_f32", "beta_f32", "c_skip_f32", "c_out_f32"):
                slot_rows(self._coeff[k], slot, fbs).copy_(slot_rows(new[k], slot, fbs))
            slot_rows(self._ts_batch, slot, fbs).copy_(slot_rows(new_ts, slot, fbs))
            # the batched-ts cache of cfg full/initialize is a separate cat
            # buffer: same rows, in place (the static-temb fast path keys on
            # the tensor's identity)
            ts_unet = self._unet_batch_timesteps()
            if ts_unet is not self._ts_batch:
                lead = ts_unet.shape[0] - new_ts.shape[0]
                src = torch.cat([new_ts[:lead], new_ts], dim=0)
                slot_rows(ts_unet, slot, fbs).copy_(slot_rows(src, slot, fbs))
            # same inputs give the other rows the values they hold
            self._refresh_temb_static()
        self._set_ctl(slot, t_index_list=list(t_index_list))

    @torch.no_grad()
    def reset_slot(self, slot: int) -> None:
        """Hand a slot to a new session: its in-flight latents and RCFG
        stock rows go back to their post-prepare() state and its controls
        to the replica defaults, so nothing of the previous tenant is
        decoded into the new session's frames. The next call is also never
        a similarity-filter skip (_prev_out is dropped), since a skip would
        return the previous tenant's last frame. Not touched: the pipelined
        ping-pong output buffers, which hold the last frame decoded for this
        slot until the slot's next frame replaces it; they are only ever
        handed out as the result of a call, which overwrites them first."""
        self._check_slot(slot)
        if slot is None:
            raise ValueError("reset_slot needs a slot")
        fbs = self.cfg.frame_buffer_size
        with self._row_writes():
            if self._x_t_buffer.shape[0]:
                slot_rows(self._x_t_buffer, slot, fbs).zero_()
            if self._canny and self._hint_feat_buffer.shape[0]:
                # the previous tenant's edges must not condition the new one
                slot_rows(self._hint_feat_buffer, slot, fbs).zero_()
            stock = self.rcfg.stock_noise
            if stock is not None and stock.shape == self._init_noise.shape:
                slot_rows(stock, slot, fbs).copy_(slot_rows(self._init_noise, slot, fbs))
        # controls: only what the previous tenant moved is rewritten
        d, c = self._slot_defaults(), self._slot_ctl[slot]
        if c["prompt"] != d["prompt"]:
            self.update_prompt(d["prompt"], slot)
        if c["negative_prompt"] != d["negative_prompt"]:
            self.update_negative_prompt(d["negative_prompt"], slot)
        if (c["guidance_scale"], c["delta"]) != (d["guidance_scale"], d["delta"]):
            self.update_guidance(d["guidance_scale"], d["delta"], slot)
        if c["t_index_list"] != d["t_index_list"]:
            self.update_t_index_list(d["t_index_list"], slot)
        if self._canny and (c["canny_low"], c["canny_high"]) != (
                d["canny_low"], d["canny_high"]):
            self.update_canny(d["canny_low"], d["canny_high"], slot)
        if self._clip_safety and c["safety_adjustment"] != d["safety_adjustment"]:
            self.update_safety(d["safety_adjustment"], slot)
        if self._lora_bank is not None and (c["lora"], c["lora_scale"]) != (
                d["lora"], d["lora_scale"]):
            self.update_lora(adapter=d["lora"], scale=d["lora_scale"], slot=slot)
        self._prev_out = None
        self._prev_sizes = None
        if slot < len(self._out_size):
            self._out_size = list(self._out_size)
            self._out_size[slot] = None
        if slot < len(self._src_size):
            self._src_size[slot] = None
        if slot < len(self._src_format):
            self._src_format[slot] = None

    @torch.no_grad()
    def update_t_index_list(self, t_index_list: Sequence[int],
                            slot: Optional[int] = None) -> None:
        """Contract of reference lib/wrapper.py:389-407: no-op when
        unchanged; length changes require prepare() (batch shape changes).
        A per-slot list must keep the length (ValueError otherwise)."""
        self._check_slot(slot)
        try:
            t_index_list = [int(t) for t in t_index_list]
        except TypeError as e:
            raise ValueError(f"t_index_list must be a list of ints: {e}") from e
        try:
            self.scheduler.sub_timesteps(t_index_list)
        except IndexError as e:
            raise ValueError(
                f"t_index_list {t_index_list} indexes outside the "
                f"{len(self.scheduler.timesteps)}-step timetable") from e
        if slot is not None:
            if t_index_list != self._slot_ctl[slot]["t_index_list"]:
                self._update_slot_t_index_list(t_index_list, slot)
            return
        if (t_index_list == self.cfg.t_index_list
                and all(c["t_index_list"] == t_index_list for c in self._slot_ctl)):
            return
        if len(t_index_list) != len(self.cfg.t_index_list):
            self._reprepare(t_index_list=t_index_list)
            return
        self.cfg.t_index_list = t_index_list
        self._set_ctl(None, t_index_list=list(t_index_list))
        new = self.scheduler.coefficients(
            t_index_list, self.cfg.frame_buffer_size, self.device, self.dtype
        )
        with self._row_writes(*self._tensors_of(new)):
            for k in ("alpha_prod_t_sqrt", "beta_prod_t_sqrt", "c_skip", "c_out"):
                self._coeff[k].copy_(new[k])
            self._coeff["sub_timesteps"] = new["sub_timesteps"]
            self._ts_batch.copy_(new["sub_timesteps_tensor"].to(self.device))
            for k in ("alpha_f32", "beta_f32", "c_skip_f32", "c_out_f32"):
                self._coeff[k].copy_(new[k].to(self.device))
            # static time-embedding caches follow the new timesteps (in place —
            # any captured graph reads the same storage). The batched-ts cache
            # is a SEPARATE cat buffer for cfg full/initialize: rebuild it.
            self._ts_unet_cache = None
            self._refresh_temb_static()

    # ------------------------------------------------------------------
    # core step (graph-capturable: static shapes, static buffers)
    # ------------------------------------------------------------------
    def _unet_batch_input(self, x_t: torch.Tensor) -> torch.Tensor:
        cfg = self.cfg
        if cfg.cfg_type == "full" and self.rcfg.active:
            return torch.cat([x_t, x_t], dim=0)
        if cfg.cfg_type == "initialize" and self.rcfg.active:
            return torch.cat([x_t[: cfg.frame_buffer_size], x_t], dim=0)
        return x_t

    def _unet_batch_embeds(self) -> torch.Tensor:
        cfg = self.cfg
        if cfg.cfg_type == "full" and self.rcfg.active:
            return self._embeds_full
        if cfg.cfg_type == "initialize" and self.rcfg.active:
            return torch.cat(
                [self._embeds_batch[: cfg.frame_buffer_size], self._embeds_batch], dim=0
            )
        return self._embeds_batch

    def _unet_batch_timesteps(self) -> torch.Tensor:
        # cached: the static-timestep UNet fast path identity-checks this
        # exact tensor object (prepare()/t-index updates reset the cache)
        t = getattr(self, "_ts_unet_cache", None)
        if t is not None:
            return t
        cfg = self.cfg
        if cfg.cfg_type == "full" and self.rcfg.active:
            t = torch.cat([self._ts_batch, self._ts_batch], dim=0)
        elif cfg.cfg_type == "initialize" and self.rcfg.active:
            t = torch.cat([self._ts_batch[: cfg.frame_buffer_size], self._ts_batch], dim=0)
        else:
            t = self._ts_batch
        self._ts_unet_cache = t
        return t

    def _refresh_temb_static(self) -> None:
        """(Re)compute the UNet's static time-embedding caches — call after
        anything that changes timesteps, added-cond or weights. In-place
        when shapes match, so captured graphs keep reading the same
        storage."""
        cfg = self.cfg
        ts = self._unet_batch_timesteps()
        added = self._added_cond
        if added is not None and (cfg.cfg_type in ("full", "initialize") and self.rcfg.active):
            extra = added.shape[0] if cfg.cfg_type == "full" else cfg.frame_buffer_size
            added = torch.cat([added[:extra], added], dim=0)
        self.unet.precompute_time_embeddings(ts, added, dtype=self.dtype)

    @torch.no_grad()
    @torch.no_grad()
    def _fp8_quality_snr(self) -> float:
        """SNR (dB) of the fp8 UNet forward vs the f16 forward on the same
        inputs — a pure function of the UNet (no engine state mutated)."""
        unet_in = self._unet_batch_input(self._init_noise)
        ts = self._unet_batch_timesteps()
        emb = self._unet_batch_embeds()
        added = self._added_cond
        cfg = self.cfg
        if added is not None and (cfg.cfg_type in ("full", "initialize") and self.rcfg.active):
            extra = added.shape[0] if cfg.cfg_type == "full" else cfg.frame_buffer_size
            added = torch.cat([added[:extra], added], dim=0)
        scales = [n._fp8_scale for n in self._fp8_norms]
        for n in self._fp8_norms:
            n._fp8_scale = None
        ref = self.unet(unet_in, ts, emb, added_cond=added).float()
        for n, s in zip(self._fp8_norms, scales):
            n._fp8_scale = s
        got = self.unet(unet_in, ts, emb, added_cond=added).float()
        err = ((got - ref) ** 2).mean().item()
        sig = (ref ** 2).mean().item()
        return 10.0 * math.log10(sig / max(err, 1e-20))

    @torch.no_grad()
    def _fp8_vae_snr(self) -> float:
        """min SNR of the fp8 TAESD decode (random latent) and encode
        (random frame) vs f16 — pure functions of the VAE."""
        g = torch.Generator(device="cpu").manual_seed(self.cfg.seed + 7)
        lat = torch.randn((1, self.cfg.latent_height, self.cfg.latent_width, 4),
                          generator=g).to(self.device, self.dtype)
        img = (torch.rand((1, self.cfg.height, self.cfg.width, 3),
                          generator=g) * 2 - 1).to(self.device, self.dtype)
        scales = [(c, c._fp8_in_scale, c._fp8_out_scale)
                  for c in self._fp8_vae["convs"]]
        for c, _, _ in scales:
            c._fp8_in_scale = c._fp8_out_scale = None
        ref_d = self.vae.decode(lat).float()
        ref_e = self.vae.encode(img).float()
        for c, si, so in scales:
            c._fp8_in_scale, c._fp8_out_scale = si, so
        got_d = self.vae.decode(lat).float()
        got_e = self.vae.encode(img).float()

        def snr(got, ref):
            err = ((got - ref) ** 2).mean().item()
            return 10.0 * math.log10((ref ** 2).mean().item() / max(err, 1e-20))

        return min(snr(got_d, ref_d), snr(got_e, ref_e))

    def _fp8_freeze(self) -> None:
        """End calibration: freeze per-layer scales, run the quality gates
        (UNet forward + TAESD decode), fall back to f16 if either fails
        (SURVEY.md §6 quality guard)."""
        log = logging.getLogger("airtc.engine")
        cfg = self.cfg
        for nrm in self._fp8_norms:
            nrm._fp8_calibrate = False
            if nrm._fp8_amax > 0:
                nrm._fp8_scale = nrm._fp8_amax * cfg.fp8_margin / 448.0
        for c in self._fp8_vae["convs"]:
            c._fp8_calibrate = False
            if c._fp8_in_amax > 0:
                c._fp8_in_scale = c._fp8_in_amax * cfg.fp8_margin / 448.0
        for c in self._fp8_vae["outs"]:
            if c._fp8_out_amax > 0:
                c._fp8_out_scale = c._fp8_out_amax * cfg.fp8_margin / 448.0
        self.fp8_snr_db = self._fp8_quality_snr()
        vae_snr = self._fp8_vae_snr() if self._fp8_vae["convs"] else 1e9
        if self.fp8_snr_db < cfg.fp8_min_snr_db or vae_snr < cfg.fp8_min_snr_db:
            for nrm in self._fp8_norms:
                nrm._fp8_scale = None
            for c in self._fp8_vae["convs"]:
                c._fp8_in_scale = c._fp8_out_scale = None
            self.fp8_active = False
            log.warning(
                "fp8 quality gate FAILED (unet %.1f dB, vae %.1f dB, "
                "min %.1f) — serving f16",
                self.fp8_snr_db, vae_snr, cfg.fp8_min_snr_db)
        else:
            self.fp8_active = True
            log.info(
                "fp8 tier active: %d GN->conv pairs + %d VAE convs, "
                "unet %.1f dB / vae %.1f dB",
                len(self._fp8_norms), len(self._fp8_vae["convs"]),
                self.fp8_snr_db, vae_snr)

    @torch.no_grad()
    def _denoise_core(self) -> torch.Tensor:
        """Stream-batch round WITHOUT the VAE decode: _img_in -> denoised
        latent (fbs, lh, lw, 4). Split out so the decode half can run on a
        second HIP stream overlapped with the next frame's denoise."""
        cfg = self.cfg
        fbs = cfg.frame_buffer_size
        co = self._coeff

        if cfg.mode == "img2img":
            # preprocess lives INSIDE the graph: _frame_in (u8) is the only
            # per-frame input buffer
            self._img_proc = ops.preprocess_from_u8(self._frame_in, self.dtype)
            x0 = self.vae.encode(self._img_proc)
            x_t0 = ops.sched_add_noise(
                x0,
                self._init_noise[:fbs],
                co["alpha_f32"][:fbs],
                co["beta_f32"][:fbs],
            ) if cfg.do_add_noise else x0
        else:  # txt2img: stage-0 input is pure noise
            x_t0 = self._init_noise[:fbs]

        x_t = torch.cat([x_t0, self._x_t_buffer], dim=0) if self._x_t_buffer.shape[0] else x_t0

        added = self._added_cond
        if added is not None and (cfg.cfg_type in ("full", "initialize") and self.rcfg.active):
            extra = added.shape[0] if cfg.cfg_type == "full" else fbs
            added = torch.cat([added[:extra], added], dim=0)
        unet_in = self._unet_batch_input(x_t)
        unet_ts = self._unet_batch_timesteps()
        unet_emb = self._unet_batch_embeds()
        control = None
        if self._canny:
            # per-stage hints: the edge map of the fbs NEW frames is encoded
            # once; the in-flight stages read the features their frames were
            # encoded to, kept stage-major exactly like x_t
            hint0 = ops.canny_hint(self._frame_in, self._canny_thr,
                                   cfg.canny_reach, self.dtype)
            feat0 = self.controlnet.hint_encoder(hint0)
            buf = self._hint_feat_buffer
            feat = torch.cat([feat0, buf], dim=0) if buf.shape[0] else feat0
            # the extra RCFG rows mirror _unet_batch_input
            if cfg.cfg_type == "full" and self.rcfg.active:
                unet_feat = torch.cat([feat, feat], dim=0)
            elif cfg.cfg_type == "initialize" and self.rcfg.active:
                unet_feat = torch.cat([feat[:fbs], feat], dim=0)
            else:
                unet_feat = feat
            control = self.controlnet(
                unet_in, unet_ts, unet_emb, scale=cfg.controlnet_scale,
                hint_features=unet_feat,
            )
            if buf.shape[0]:
                # stage i's features become stage i+1's, in step with the
                # latent shift below
                buf.copy_(feat[:-fbs])
        elif self.controlnet is not None and cfg.mode == "img2img":
            # processor "none": hint = the current input frame (per
            # in-flight stage we reuse the newest frame's hint; the canny
            # branch above keeps per-stage hints in a FIFO mirroring the
            # latent buffer)
            hint = self._img_proc.expand(unet_in.shape[0], -1, -1, -1).contiguous()
            control = self.controlnet(
                unet_in, unet_ts, unet_emb, hint, scale=cfg.controlnet_scale
            )
        eps = self.unet(unet_in, unet_ts, unet_emb, added_cond=added, control=control)
        eps = self.rcfg.apply(eps, fbs)
        # fused LCM step (one kernel; same math as scheduler.step_batch)
        denoised = ops.sched_blend(x_t, eps, co["alpha_f32"], co["beta_f32"],
                                   co["c_out_f32"], co["c_skip_f32"])

        if denoised.shape[0] > fbs:
            # shift: stage i output -> stage i+1 input at tau_{i+1}
            nxt = ops.sched_add_noise(
                denoised[:-fbs].contiguous(),
                self._init_noise[fbs:],
                co["alpha_f32"][fbs:],
                co["beta_f32"][fbs:],
            ) if cfg.do_add_noise else denoised[:-fbs]
            self._x_t_buffer.copy_(nxt)

        return denoised[-fbs:]

    @torch.no_grad()
    def _decode_core(self, latent: torch.Tensor) -> torch.Tensor:
        decoded = self.vae.decode(latent)
        if self._clip_safety:
            # patches -> tower -> head -> black, all on the device and in
            # the decoder's image, so RGB, I420 and source-size egress
            # inherit the verdict
            decoded = self.safety_checker.filter_(
                decoded.contiguous(), self._safety_adjust, self._safety_count)
        elif self.safety_checker is not None:
            decoded = self.safety_checker.filter(decoded)
        if self.cfg.output_format == "i420" and not self._egress:
            # same launch count: the u8 rounding and the colour conversion
            # are one kernel
            return ops.postprocess_to_i420(decoded)
        # source-size egress resizes packed RGB: there the colour conversion
        # belongs to the egress step and the graph is the RGB one
        return ops.postprocess_to_u8(decoded)

    @torch.no_grad()
    def _step_core(self) -> torch.Tensor:
        """Sequential full step (CPU / eager GPU path)."""
        return self._decode_core(self._denoise_core())

    def _maybe_capture(self) -> None:
        """Capture the per-frame step into hipGraphs (torch.cuda.CUDAGraph is
        hipGraph on ROCm).

        PIPELINED mode (default): the step is split into two graphs —
        g1 = preprocess-side denoise (VAE encode -> stream-batch UNet ->
        scheduler -> latent handoff buffer) on stream A, and
        g2 = VAE decode + postprocess on stream B. g2(frame i) runs
        CONCURRENTLY with g1(frame i+1): steady-state throughput becomes
        max(g1, g2) instead of g1+g2. Latent handoff buffers are ping-pong
        (two g1/g2 captures sharing pools per stream); event chain:
          sA: wait done[pp] -> g1 -> record lat[pp]
          sB: wait lat[pp]  -> g2 -> record done[pp]
        The CALLER's stream is never made to wait (that would transitively
        serialise the next frame's g1 behind this frame's decode) —
        consumers that read the output tensor call sync_output() first.
        """
        if (
            self._graph is not None
            or self.device.type != "cuda"
            or not self.cfg.use_hip_graph
        ):
            return
        fbs = self.cfg.frame_buffer_size
        lh, lw = self.cfg.latent_height, self.cfg.latent_width
        # pipeline overlap composes with the similarity filter: a skipped
        # frame simply returns the persistent output buffer of the last
        # replay without touching the stream A/B event chain
        self._pipelined = self.cfg.pipeline_overlap
        sA = torch.cuda.Stream()
        sB = torch.cuda.Stream()
        self._sA, self._sB = sA, sB
        self._lat_out = [
            torch.zeros((fbs, lh, lw, 4), device=self.device, dtype=self.dtype)
            for _ in range(2)
        ]
        # warmup (weight-transform caches etc.) on a side stream
        sA.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(sA):
            # the warmup decodes are nobody's frames: keep them out of the
            # clip checker's flagged-frame counts
            counts = self._safety_count.clone() if self._clip_safety else None
            for _ in range(2):
                lat = self._denoise_core()
                self._lat_out[0].copy_(lat)
                _ = self._decode_core(self._lat_out[0])
            if counts is not None:
                self._safety_count.copy_(counts)
        torch.cuda.current_stream().wait_stream(sA)

        if not self._pipelined:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=sA):
                self._graph_out = self._step_core()
            self._graph = g
            return

        self._g1, self._g2, self._out_u8 = [], [], []
        for pp in range(2):
            g1 = torch.cuda.CUDAGraph()
            kw = {"pool": self._g1[0].pool()} if pp else {}
            with torch.cuda.graph(g1, stream=sA, **kw):
                self._lat_out[pp].copy_(self._denoise_core())
            self._g1.append(g1)
            g2 = torch.cuda.CUDAGraph()
            kw = {"pool": self._g2[0].pool()} if pp else {}
            with torch.cuda.graph(g2, stream=sB, **kw):
                self._out_u8.append(self._decode_core(self._lat_out[pp]))
            self._g2.append(g2)
        self._ev_in = torch.cuda.Event()
        self._ev_lat = [torch.cuda.Event() for _ in range(2)]
        self._ev_done = [torch.cuda.Event() for _ in range(2)]
        for e in self._ev_done:
            e.record(sB)
        self._pp = 0
        self._graph = True  # sentinel: pipelined graphs ready

    def sync_output(self) -> None:
        """Make the caller's stream wait until the last returned output is
        fully produced (pipelined mode defers this so the next frame's
        denoise can overlap the decode)."""
        ev = getattr(self, "_last_done", None)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    # ------------------------------------------------------------------
    # public frame API
    # ------------------------------------------------------------------
    def _fit_into(self, srcs, out: torch.Tensor) -> None:
        """Write every slot of `out` (fbs, H, W, 3) from its source frame on
        the current stream: engine-sized sources are copied, any other size
        goes through the fused crop+resize kernel (ops.fit_frame_u8)."""
        shape = out.shape[1:]
        for b, src in enumerate(srcs):
            if src.shape == shape:
                out[b].copy_(src)
            else:
                ops.fit_frame_u8(src, out, b, self.cfg.fit_mode)

    def _load_frame_in(self, frame_u8, srcs, stream=None) -> None:
        """Fill the static input slot on the current stream. `srcs` is None
        on the equal-size path (one plain copy, as ever). Otherwise it holds
        one device frame per slot and each is fitted STRAIGHT INTO
        _frame_in[b] by the stream that owns _frame_in. In pipelined mode
        that is stream A, after its wait on _ev_in (upload finished) and
        _ev_done (previous replays done), so the fit is ordered against the
        g1 replay that reads the slot exactly as the plain copy is. There is
        deliberately no staging buffer on the caller's stream: the caller
        runs ahead of stream A, and frame i+1's fit would overwrite a shared
        staging buffer before stream A had consumed frame i. The sources
        were allocated on the caller's stream, hence record_stream."""
        if srcs is None:
            self._frame_in.copy_(frame_u8)
            if stream is not None:
                frame_u8.record_stream(stream)
            return
        self._fit_into(srcs, self._frame_in)
        if stream is not None:
            for src in srcs:
                src.record_stream(stream)

    def _i420_to_rgb_sources(self, frame_u8):
        """Replace every I420 source (ops/interface.py: a 2-D (3Hs/2, Ws)
        frame, a (fbs, 3Hs/2, Ws) batch, or such entries of a list) by its
        RGB conversion on the device: uploaded at 1.5 B/px and converted
        with ops.i420_to_rgb_u8 on the caller's stream right after the
        upload. What comes back is what __call__ has always taken, so
        everything downstream (equal-size copy, fit, similarity filter, the
        stream A/B chain) is untouched. Returns (frames, per-slot formats)."""
        def convert(t):
            return ops.i420_to_rgb_u8(t.to(self.device, non_blocking=True))

        def check_2d(t):
            if not ops.is_i420(t):
                raise ValueError(
                    f"2-D frames must be I420 (3H/2, W) uint8 with even H, W, "
                    f"got {tuple(t.shape)} {t.dtype}")

        if isinstance(frame_u8, (list, tuple)):
            fmts = ["i420" if t.dim() == 2 else "rgb" for t in frame_u8]
            if "i420" not in fmts:
                return frame_u8, fmts
            out = []
            for t in frame_u8:
                if t.dim() == 2:
                    check_2d(t)
                    t = convert(t)
                out.append(t)
            return out, fmts
        if frame_u8.dim() == 2:
            check_2d(frame_u8)
            return convert(frame_u8), ["i420"]
        if frame_u8.dim() == 3 and frame_u8.shape[-1] != 3:
            if not ops.is_i420(frame_u8):
                raise ValueError(
                    f"3-D frames must be (H,W,3) RGB or an I420 batch "
                    f"(fbs, 3H/2, W) uint8, got {tuple(frame_u8.shape)} {frame_u8.dtype}")
            return convert(frame_u8), ["i420"] * frame_u8.shape[0]
        n = 1 if frame_u8.dim() == 3 else frame_u8.shape[0]
        return frame_u8, ["rgb"] * n

    def _egress_targets(self) -> list:
        """Per slot ((ry, rx, rh, rw), (Ht, Wt)): the window of the engine
        frame that goes back to the slot's session and the size it goes back
        at, from the source sizes of this call."""
        cfg = self.cfg
        return [
            ops.unfit_geometry(sz[0], sz[1], cfg.height, cfg.width,
                               cfg.fit_mode, even=cfg.output_format == "i420",
                               max_side=cfg.output_max_side)
            for sz in self._src_size
        ]

    def _egress_frames(self, frames: torch.Tensor, targets: list) -> list:
        """The egress step: one fresh tensor per slot out of the finished
        (fbs, H, W, 3) u8 frames, on the current stream. A slot that reads
        the whole frame at engine size gets exactly what output_size ==
        "engine" returns (a copy, or its colour conversion); every other
        slot is ONE launch of ops.unfit_frame_u8, which for I420 resizes
        and converts together."""
        H, W = int(frames.shape[1]), int(frames.shape[2])
        fmt = self.cfg.output_format
        outs = []
        for b, (window, size) in enumerate(targets):
            if tuple(window) == (0, 0, H, W) and tuple(size) == (H, W):
                outs.append(ops.rgb_u8_to_i420(frames[b]) if fmt == "i420"
                            else frames[b].clone())
            else:
                outs.append(ops.unfit_frame_u8(frames[b], window, size, fmt))
        return outs

    @torch.no_grad()
    def __call__(self, frame_u8) -> torch.Tensor:
        """frame_u8: (H,W,3) or (fbs,H,W,3) uint8 RGB on any device, or a
        list/tuple of fbs (Hs,Ws,3) frames of differing sizes. Frames whose
        size is not the engine's (cfg.height, cfg.width) are uploaded at
        source size and fitted on the device (cfg.fit_mode). Any source may
        instead be an I420 frame ((3Hs/2,Ws), a (fbs,3Hs/2,Ws) batch, or
        list entries of either format): it is converted on the device.
        Returns stylised (H,W,3) / (fbs,H,W,3) uint8 RGB on self.device, or
        (3H/2,W) / (fbs,3H/2,W) I420 with cfg.output_format == "i420".
        With cfg.output_size == "source" every slot comes back at the size
        its source had (ops.unfit_geometry): one tensor for a single-frame
        call, else a list of fbs tensors whose sizes may differ."""
        assert self._prepared, "call prepare() first"
        cfg = self.cfg
        eng_shape = (cfg.height, cfg.width, 3)
        frame_u8, src_format = self._i420_to_rgb_sources(frame_u8)
        # srcs: per-slot source frames when any of them needs fitting;
        # None = everything is engine-sized (the path is what it always was)
        srcs = None
        if isinstance(frame_u8, (list, tuple)):
            squeeze = False
            if len(frame_u8) != cfg.frame_buffer_size:
                raise ValueError(
                    f"expected {cfg.frame_buffer_size} frames, got {len(frame_u8)}")
            if all(tuple(t.shape) == eng_shape for t in frame_u8):
                frame_u8 = torch.stack(
                    [t.to(self.device, non_blocking=True) for t in frame_u8])
            else:
                srcs = list(frame_u8)
        else:
            squeeze = frame_u8.dim() == 3
            if squeeze:
                frame_u8 = frame_u8.unsqueeze(0)
            if tuple(frame_u8.shape[1:]) != eng_shape:
                if frame_u8.shape[0] != cfg.frame_buffer_size:
                    raise ValueError(
                        f"expected {cfg.frame_buffer_size} frames, got {frame_u8.shape[0]}")
                srcs = list(frame_u8.unbind(0))

        with self.timers.stage("preprocess"):
            if srcs is None:
                frame_u8 = frame_u8.to(self.device, non_blocking=True)
                self._src_size = [eng_shape[:2]] * frame_u8.shape[0]
            else:
                for t in srcs:
                    if t.dim() != 3 or t.shape[-1] != 3 or t.dtype != torch.uint8:
                        raise ValueError(
                            f"frames must be (Hs,Ws,3) uint8, got {tuple(t.shape)} {t.dtype}")
                srcs = [t.to(self.device, non_blocking=True) for t in srcs]
                self._src_size = [(int(t.shape[0]), int(t.shape[1])) for t in srcs]
                if self.sim_filter is not None:
                    # the filter must see the FITTED frame (its signature
                    # then never depends on the source resolution) and it
                    # decides before stream A is touched: fit into a fresh
                    # per-call tensor on the caller's stream and continue
                    # on the equal-size path (no shared staging: each call
                    # owns its tensor, record_stream covers stream A)
                    frame_u8 = torch.empty_like(self._frame_in)
                    self._fit_into(srcs, frame_u8)
                    srcs = None

        self._src_format = src_format
        targets = self._egress_targets() if self._egress else None
        sizes = [list(t[1]) for t in targets] if self._egress else None
        if self.sim_filter is not None and self._prev_out is not None:
            # on-device pooled cosine (centering + 64x64 avg-pool inside
            # the filter); the only CPU sync is one scalar read that waits
            # on the frame upload, NOT on the pipelined streams. The filter
            # sees every frame, but a skip stands only while every slot
            # still wants the size _prev_out was made at
            if self.sim_filter.should_skip(frame_u8) and sizes == self._prev_sizes:
                out = self._prev_out
                self.timers.frame_done()
                return out[0] if squeeze else out

        with self.timers.stage("diffusion"):
            if (self.device.type == "cuda" and self.cfg.use_hip_graph
                    and not self._fp8_calib_left):
                self._maybe_capture()
                if self._pipelined:
                    cur = torch.cuda.current_stream()
                    pp = self._pp
                    self._pp ^= 1
                    self._ev_in.record(cur)
                    with torch.cuda.stream(self._sA):
                        self._sA.wait_event(self._ev_in)
                        self._sA.wait_event(self._ev_done[pp])
                        self._load_frame_in(frame_u8, srcs, self._sA)
                        self._g1[pp].replay()
                        self._ev_lat[pp].record()
                    with torch.cuda.stream(self._sB):
                        self._sB.wait_event(self._ev_lat[pp])
                        self._g2[pp].replay()
                        out = self._out_u8[pp]
                        if self._egress:
                            # stream B owns the frame it just decoded: the
                            # egress reads it here, before done[pp], so
                            # sync_output() covers the resized frames too
                            out = self._egress_frames(out, targets)
                        self._ev_done[pp].record()
                    self._last_done = self._ev_done[pp]
                    if self._egress:
                        # allocated on stream B, read on the caller's (the
                        # mirror of _load_frame_in's sources)
                        for t in out:
                            t.record_stream(cur)
                else:
                    self._load_frame_in(frame_u8, srcs)
                    self._graph.replay()
                    out = self._graph_out
                    if self._egress:
                        out = self._egress_frames(out, targets)
            else:
                self._load_frame_in(frame_u8, srcs)
                out = self._step_core()
                if self._egress:
                    out = self._egress_frames(out, targets)
                if self._fp8_calib_left:
                    self._fp8_calib_left -= 1
                    if self._fp8_calib_left == 0:
                        self._fp8_freeze()

        self._prev_out = out
        if self._egress:
            self._prev_sizes = sizes
            self._out_size = sizes
        self.timers.frame_done()
        return out[0] if squeeze else out

    # reference wrapper exposes explicit img2img/txt2img entry points
    @torch.no_grad()
    def img2img(self, frame_u8: torch.Tensor) -> torch.Tensor:
        assert self.cfg.mode == "img2img"
        return self(frame_u8)

    @torch.no_grad()
    def txt2img(self) -> torch.Tensor:
        assert self.cfg.mode == "txt2img"
        fbs = self.cfg.frame_buffer_size
        dummy = torch.zeros(
            (fbs, self.cfg.height, self.cfg.width, 3), dtype=torch.uint8, device=self.device
        )
        return self(dummy)

    def stats(self) -> dict:
        d = self.timers.snapshot()
        d["ingest"] = {
            "fit_mode": self.cfg.fit_mode,
            "engine_size": [self.cfg.height, self.cfg.width],
            # last source [height, width] per slot (None: no frame yet)
            "last_source_size": [
                None if sz is None else list(sz)
                for sz in getattr(self, "_src_size", [])
            ],
        }
        fmts = getattr(self, "_src_format", [])
        if self.cfg.output_format == "i420" or "i420" in fmts:
            self._yuv_seen = True
        if getattr(self, "_yuv_seen", False):
            # "rgb" / "i420" as last handed in per slot (None: no frame
            # yet). Reported once YUV is in play (I420 output configured or
            # an I420 frame seen), so RGB-only deployments keep the ingest
            # record they had
            d["ingest"]["source_format"] = list(fmts)
        if self.cfg.output_size == "source":
            d["egress"] = {
                "output_size": self.cfg.output_size,
                "max_side": self.cfg.output_max_side,
                # last returned [height, width] per slot (None: no frame yet)
                "last_output_size": [
                    None if sz is None else list(sz)
                    for sz in getattr(self, "_out_size", [])
                ],
            }
        if getattr(self, "_canny", False):
            d["controlnet"] = {
                "processor": self.cfg.controlnet_processor,
                "scale": float(self.cfg.controlnet_scale),
                "canny_reach": self.cfg.canny_reach,
                # [low, high] per slot, as last written
                "canny_thresholds": [
                    [c["canny_low"], c["canny_high"]] for c in self._slot_ctl],
            }
        if self._clip_safety and getattr(self, "_safety_adjust", None) is not None:
            d["safety"] = {
                "arch": "clip-vit",
                "config": dataclasses.asdict(self.safety_checker.cfg),
                "weights": self.safety_checker.weights,
                # per slot, as last written (host-side copies)
                "adjustment": [c["safety_adjustment"] for c in self._slot_ctl],
                # per slot; the one device read, made here and never in the
                # frame path
                "frames_flagged": self._safety_count.tolist(),
            }
        if self._lora_bank is not None:
            d["lora"] = {
                "capacity": self.cfg.lora_adapters,
                "max_rank": self.cfg.lora_max_rank,
                # name -> bank index and how often the name was loaded
                "loaded": {n: {"index": i, "loads": self._lora_loads.get(n, 0)}
                           for n, i in self._lora_names.items()},
                # per slot, as last written (host-side copies)
                "slots": [{"lora": self._lora_name_of(c["lora"]),
                           "index": c["lora"], "scale": c["lora_scale"]}
                          for c in self._slot_ctl],
            }
        if self.cfg.use_fp8:
            d["fp8"] = {
                "active": self.fp8_active,
                "layers": len(self._fp8_norms),
                "vae_convs": len(self._fp8_vae["convs"]),
                "quality_snr_db": self.fp8_snr_db,
                "calibrating": self._fp8_calib_left > 0,
            }
        return d
