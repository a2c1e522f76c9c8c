"""LoRA loading & weight fusion.

Parity target: the reference fuses LCM-LoRA plus an arbitrary dict of LoRA
files with per-file scales at engine build time (reference
lib/wrapper.py:645-697; build.py:18-32 uses a Civitai "ghibli" LoRA at scale
1.0; download.py:23-41 fetches it). Fusion happens BEFORE kernel-plan
capture, so the hot path never sees LoRA math — same design as the
reference's TRT engines compiled from the fused model.

Formats: a state dict of (down, up, alpha) triples keyed like
"<module_path>.lora_down.weight" / ".lora_up.weight" / ".alpha"
(kohya-style), or "<module_path>.lora_A.weight"/"lora_B.weight" (PEFT-style).
Module paths are matched against named_modules() of our UNet.

W_fused = W + scale * (alpha/rank) * (up @ down)
"""
from __future__ import annotations

import contextlib
import math
import re
from typing import Dict

import torch
import torch.nn as nn


def _collect_pairs(sd: Dict[str, torch.Tensor]) -> Dict[str, dict]:
    out: Dict[str, dict] = {}
    for k, v in sd.items():
        for marker, slot in (
            (".lora_down.weight", "down"),
            (".lora_up.weight", "up"),
            (".lora_A.weight", "down"),
            (".lora_B.weight", "up"),
            (".alpha", "alpha"),
        ):
            if k.endswith(marker):
                base = k[: -len(marker)]
                out.setdefault(base, {})[slot] = v
                break
    return out


def fuse_lora_state_dict(
    model: nn.Module, sd: Dict[str, torch.Tensor], scale: float = 1.0
) -> int:
    """Fuse a LoRA state dict into matching Linear/Conv weights in-place.

    Returns the number of modules fused. Unmatched LoRA keys are skipped
    (the reference behaves the same: fusing is best-effort by name).
    """
    pairs = _collect_pairs(sd)
    by_name = dict(model.named_modules())
    n = 0
    for base, slots in pairs.items():
        if "down" not in slots or "up" not in slots:
            continue
        # normalise separators: kohya uses '_' where modules use '.'
        cand = [base, base.replace("lora_unet_", "").replace("_", ".")]
        target = None
        for c in cand:
            if c in by_name and hasattr(by_name[c], "weight"):
                target = by_name[c]
                break
        if target is None:
            continue
        target_dev = target.weight.device
        down = slots["down"].float().to(target_dev)
        up = slots["up"].float().to(target_dev)
        rank = down.shape[0]
        alpha = float(slots.get("alpha", torch.tensor(float(rank))))
        w = target.weight.data
        if w.dim() == 4:  # conv OIHW: lora stored as (r, I*k*k) / (O, r)
            delta = (up.flatten(1) @ down.flatten(1)).view_as(w)
        else:
            delta = up @ down
        target.weight.data = (w.float() + scale * (alpha / rank) * delta).to(w.dtype)
        n += 1
    return n


def load_lora_file(path: str) -> Dict[str, torch.Tensor]:
    """Load a .safetensors or torch-serialised LoRA file."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file

        return load_file(path)
    return torch.load(path, map_location="cpu")


def make_random_lora(
    model: nn.Module, rank: int = 4, seed: int = 0, limit: int = 8
) -> Dict[str, torch.Tensor]:
    """Synthesize a LoRA dict targeting the first `limit` Linear modules —
    offline stand-in for LCM-LoRA (no network: SURVEY.md §7 env note)."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    count = 0
    for name, m in model.named_modules():
        if count >= limit:
            break
        w = getattr(m, "weight", None)
        if w is None or w.dim() != 2:
            continue
        o, i = w.shape
        sd[f"{name}.lora_down.weight"] = torch.randn(rank, i, generator=g) * 0.01
        sd[f"{name}.lora_up.weight"] = torch.randn(o, rank, generator=g) * 0.01
        sd[f"{name}.alpha"] = torch.tensor(float(rank))
        count += 1
    return sd


# ---------------------------------------------------------------------------
# per-session adapters: an unfused, device-resident bank (ops.lora_delta_)
# ---------------------------------------------------------------------------

class LoraTarget:
    """One targeted projection: its slice of the bank and the row tables the
    kernel reads. A (n, R, K) and B (n, N, R) hold, per bank index, the
    adapter in the layout of the tensor the projection's GEMM really
    consumes and produces (head padding applied)."""

    __slots__ = ("A", "B", "rows", "pad_out", "pad_in", "shape")

    def __init__(self, A, B, rows, pad_out, pad_in, shape):
        self.A, self.B, self.rows = A, B, rows
        self.pad_out, self.pad_in = pad_out, pad_in
        self.shape = shape  # the file-side (out, in) of the Linear

    def apply_(self, y: torch.Tensor, x: torch.Tensor, col_offset: int = 0,
               rows=None) -> torch.Tensor:
        """y[..., col_offset : col_offset+N] += the rows' adapter deltas, in
        place. rows: (row_adapter, row_scale) of x's batch; default the
        engine's shared tables, whose first x.shape[0] entries follow the
        row law (row % fbs == slot) in every UNet batch layout."""
        from .. import ops

        if x.dim() != 3 or y.dim() != 3:
            raise ValueError(
                "a LoRA-targeted projection takes (batch, tokens, channels), "
                f"got x {tuple(x.shape)}, y {tuple(y.shape)}")
        ra, rs = self.rows if rows is None else rows
        bt = x.shape[0]
        if ra.shape[0] < bt:
            raise ValueError(
                f"LoRA row table holds {ra.shape[0]} rows, the batch has {bt}")
        if not x.is_contiguous():
            # every x the UNet hands a target is contiguous; this copy only
            # serves a caller outside it
            x = x.contiguous()
        return ops.lora_delta_(y, x, self.A, self.B, ra[:bt], rs[:bt],
                               col_offset)


def lora_name_table(cfg) -> Dict[str, str]:
    """Every spelling of a UNet module path a LoRA file may use -> our module
    path: diffusers paths (PEFT, after the "unet." prefix), their kohya
    flattening (lora_unet_<path with dots as underscores>), and our own."""
    from .load import diffusers_unet_key_map

    table: Dict[str, str] = {}
    for src, dst in diffusers_unet_key_map(cfg):
        if not src.endswith(".weight"):
            continue
        s, d = src[: -len(".weight")], dst[: -len(".weight")]
        table[s] = d
        table["unet." + s] = d
        table["lora_unet_" + s.replace(".", "_")] = d
        table[d] = d
    return table


class LoraBank:
    """n_adapters unfused adapters over every Linear reached from a
    SpatialTransformer: attn1 / attn2 to_q, to_k, to_v, to_out, ff.proj,
    ff.out, and proj_in / proj_out where they are Linear. Zeroed at build;
    load() fills one index in place, so a captured graph that reads the bank
    follows it without a re-capture."""

    def __init__(self, unet: nn.Module, n_adapters: int, max_rank: int):
        from .unet import CrossAttention, Linear, SpatialTransformer

        if not 1 <= n_adapters <= 64:
            raise ValueError(f"n_adapters must be in [1, 64], got {n_adapters}")
        if not 1 <= max_rank <= 64:
            raise ValueError(f"max_rank must be in [1, 64], got {max_rank}")
        self.n_adapters = n_adapters
        self.max_rank = max_rank
        self.R = 16 if max_rank <= 16 else 32 if max_rank <= 32 else 64
        self.unet = unet
        self.names = lora_name_table(unet.cfg)
        self.targets: Dict[str, LoraTarget] = {}
        self.loaded: list = [False] * n_adapters
        p = next(unet.parameters())
        self.device, self.dtype = p.device, p.dtype
        # shared by every target; the engine sizes and fills them
        self.rows = [torch.full((1,), -1, dtype=torch.int32, device=self.device),
                     torch.zeros(1, dtype=torch.float32, device=self.device)]
        mods = dict(unet.named_modules())
        for tname, t in mods.items():
            if not isinstance(t, SpatialTransformer):
                continue
            for name, m in t.named_modules():
                if not isinstance(m, Linear):
                    continue
                path = f"{tname}.{name}"
                parent = mods[path.rsplit(".", 1)[0]]
                pad_out = pad_in = None
                if isinstance(parent, CrossAttention):
                    if name.endswith("to_out"):
                        pad_in = parent
                    else:
                        pad_out = parent
                o, i = m.weight.shape
                N = parent.heads * parent.dpad if pad_out is not None else o
                K = parent.heads * parent.dpad if pad_in is not None else i
                z = dict(device=self.device, dtype=self.dtype)
                tg = LoraTarget(torch.zeros(n_adapters, self.R, K, **z),
                                torch.zeros(n_adapters, N, self.R, **z),
                                self.rows, pad_out, pad_in, (o, i))
                self.targets[path] = tg
                m._lora = tg

    def set_rows(self, row_adapter: torch.Tensor, row_scale: torch.Tensor) -> None:
        """Install the (shared) row tables: every target reads these."""
        self.rows[0], self.rows[1] = row_adapter, row_scale

    def _resolve(self, base: str):
        """(kind, our path): kind in loaded-candidates 'target', 'conv',
        'text_encoder', 'unmatched'."""
        if base.startswith(("lora_te", "text_encoder.", "te.")):
            return "text_encoder", None
        ours = self.names.get(base)
        if ours is None:
            return "unmatched", None
        if ours in self.targets:
            return "target", ours
        return "conv", ours

    @torch.no_grad()
    def load(self, index: int, state_dict: Dict[str, torch.Tensor],
             scale: float = 1.0, ordered=None, after=None) -> dict:
        """Write an adapter file into bank index `index`, in place. Everything
        is validated before the first write; on an error the index is as it
        was. Targets the file does not name are zeroed. ordered: a context
        manager factory taking the staged device tensors (the engine's
        _row_writes) around the in-place copies; after: called inside it once
        the copies are enqueued."""
        if isinstance(index, bool) or not isinstance(index, int) \
                or not 0 <= index < self.n_adapters:
            raise ValueError(
                f"bank index must be an int in [0, {self.n_adapters}), got {index!r}")
        if not math.isfinite(float(scale)):
            raise ValueError(f"scale must be finite, got {scale!r}")
        counts = {"loaded": 0, "skipped_conv": 0, "skipped_text_encoder": 0,
                  "unmatched": 0}
        staged: Dict[str, tuple] = {}
        for base, slots in _collect_pairs(state_dict).items():
            if "down" not in slots or "up" not in slots:
                continue
            kind, path = self._resolve(base)
            down, up = slots["down"], slots["up"]
            if kind == "target" and (down.dim() != 2 or up.dim() != 2):
                kind = "conv"  # LoCon-style 4-d factors on a 1x1 target
            if kind == "text_encoder":
                counts["skipped_text_encoder"] += 1
                continue
            if kind == "conv":
                counts["skipped_conv"] += 1
                continue
            if kind == "unmatched":
                counts["unmatched"] += 1
                continue
            tg = self.targets[path]
            rank = down.shape[0]
            if rank > self.max_rank:
                raise ValueError(
                    f"{base}: rank {rank} exceeds the bank's max_rank "
                    f"{self.max_rank}")
            o, i = tg.shape
            if tuple(down.shape) != (rank, i) or tuple(up.shape) != (o, rank):
                raise ValueError(
                    f"{base}: down {tuple(down.shape)} / up {tuple(up.shape)} "
                    f"do not fit the target's weight ({o}, {i})")
            if path in staged:
                raise ValueError(f"{base}: a second adapter for {path}")
            alpha = float(slots.get("alpha", torch.tensor(float(rank))))
            a = down.float()
            b = up.float() * (float(scale) * alpha / rank)
            if tg.pad_out is not None:
                b = tg.pad_out._pad_heads(b)
            if tg.pad_in is not None:
                # zero input-columns at the padded head positions, as _wout
                a = tg.pad_in._pad_heads(a.t().contiguous()).t().contiguous()
            staged[path] = (a, b, rank)
            counts["loaded"] += 1
        if not staged:
            raise ValueError(
                "the adapter matches no targeted projection of this UNet "
                f"({counts})")
        # pad to the bank's layout and move to the device first (the
        # caller's stream), so that what `ordered` wraps is device-to-device
        # copies alone: nothing in it blocks the host
        ready = []
        for path, tg in self.targets.items():
            if path not in staged:
                ready.append((tg, None, None))
                continue
            a, b, rank = staged[path]
            fa = torch.zeros(tg.A.shape[1:], dtype=torch.float32)
            fb = torch.zeros(tg.B.shape[1:], dtype=torch.float32)
            fa[:rank] = a
            fb[:, :rank] = b
            ready.append((tg, fa.to(self.device, self.dtype),
                          fb.to(self.device, self.dtype)))
        with (ordered(*[t for _, a, b in ready if a is not None
                        for t in (a, b)])
              if ordered is not None else contextlib.nullcontext()):
            for tg, fa, fb in ready:
                if fa is None:
                    tg.A[index].zero_()
                    tg.B[index].zero_()
                else:
                    tg.A[index].copy_(fa)
                    tg.B[index].copy_(fb)
            if after is not None:
                after()
        self.loaded[index] = True
        return counts
