"""Residual Classifier-Free Guidance (RCFG).

From-scratch implementation of the RCFG option surface the reference exposes
through its wrapper: cfg_type in {none, full, self, initialize} with
guidance_scale and delta (reference lib/wrapper.py:61,124-127,217-219).

Semantics implemented here (our own math, locked by tests):

- none:       eps_out = eps_c. No extra UNet cost.
- full:       classic CFG — the UNet batch is doubled with uncond embeddings
              (handled by the engine); eps_out = eps_u + g (eps_c - eps_u).
- self:       Residual CFG Self-Negative: a running per-stage "stock noise"
              buffer stands in for the uncond prediction.
              eps_out = eps_c + (g - 1) (eps_c - delta * stock), and the
              stock buffer is updated from the conditional prediction as the
              stream shifts (stage i's eps becomes stage i+1's stock).
- initialize: like self, but the stock buffer is (re)seeded from a single
              uncond UNet pass on the first frame_buffer_size rows
              (engine adds those rows to the batch; see unet_batch law,
              reference lib/wrapper.py:159-163).

Per-row coefficients: once reset() has run on an active instance, guidance
and delta live in f32 (rows,) tensors next to the stock buffer and apply()
is ONE ops.rcfg_apply call (a single HIP launch on the GPU) that reads them
from memory. set_guidance() rewrites a serving slot's rows in place, so the
values change under a captured hipGraph and differ between the sessions
that share a batch. A row whose scale is <= 1 gets g - 1 = 0: its eps
passes through, the per-row form of "inactive".
"""
from __future__ import annotations

import torch

from .. import ops
from .scheduler import slot_rows


class ResidualCFG:
    def __init__(self, cfg_type: str, guidance_scale: float, delta: float = 1.0,
                 *, runtime: bool = False):
        if cfg_type not in ("none", "full", "self", "initialize"):
            raise ValueError(f"unknown cfg_type {cfg_type!r}")
        self.cfg_type = cfg_type
        self.guidance_scale = float(guidance_scale)
        self.delta = float(delta)
        # runtime: count as active whatever the scale, so the step (and for
        # full/initialize the extra UNet rows) is in the captured graph and
        # guidance can be raised later without a re-capture
        self.runtime = bool(runtime)
        self.stock_noise: torch.Tensor | None = None
        # per-row f32 coefficients (reset() allocates them): g_rows =
        # max(g, 1), gm1_rows = float32(max(g, 1) - 1.0), delta_rows
        self.g_rows: torch.Tensor | None = None
        self.gm1_rows: torch.Tensor | None = None
        self.delta_rows: torch.Tensor | None = None
        # host-side: do all rows still hold the scalars? (a per-slot write
        # clears it, a replica-wide write of both values sets it again)
        self._uniform = True

    @property
    def active(self) -> bool:
        # once the per-row tensors exist the step stays in the hot path even
        # if every row is lowered to <= 1 (its rows then pass eps through):
        # a captured graph must keep its batch layout
        return self.cfg_type != "none" and (
            self.runtime or self.gm1_rows is not None or self.guidance_scale > 1.0)

    def reset(self, init_noise: torch.Tensor) -> None:
        """Seed the stock-noise buffer (engine calls at prepare()) and, when
        active, allocate the per-row coefficients from the scalars."""
        self.stock_noise = init_noise.clone()
        self.g_rows = self.gm1_rows = self.delta_rows = None
        self._uniform = True
        if self.active:
            rows = init_noise.shape[0]
            dev = init_noise.device
            self.g_rows = torch.empty(rows, dtype=torch.float32, device=dev)
            self.gm1_rows = torch.empty(rows, dtype=torch.float32, device=dev)
            self.delta_rows = torch.empty(rows, dtype=torch.float32, device=dev)
            self.set_guidance(self.guidance_scale, self.delta)

    def set_guidance(self, guidance_scale: float | None = None,
                     delta: float | None = None, slot: int | None = None,
                     fbs: int = 1) -> None:
        """Rewrite guidance and/or delta in place: the rows of `slot`
        (row % fbs == slot) or, with slot None, every row — then the scalars
        follow too. fill_ passes the value as a kernel argument: no sync,
        and the write is ordered on the current stream."""
        if slot is not None:
            self._uniform = False
        elif self._uniform or (guidance_scale is not None and delta is not None):
            self._uniform = True
        if guidance_scale is not None:
            g = max(float(guidance_scale), 1.0)
            if self.gm1_rows is not None:
                slot_rows(self.g_rows, slot, fbs).fill_(g)
                # g - 1.0 in double, rounded to f32 by the fill: the value
                # the scalar path's (g - 1.0) * tensor multiplies by
                slot_rows(self.gm1_rows, slot, fbs).fill_(g - 1.0)
            if slot is None:
                self.guidance_scale = float(guidance_scale)
        if delta is not None:
            if self.delta_rows is not None:
                slot_rows(self.delta_rows, slot, fbs).fill_(float(delta))
            if slot is None:
                self.delta = float(delta)

    def _per_row(self, eps: torch.Tensor, extra_rows: int) -> bool:
        """Can this batch go through ops.rcfg_apply? The coefficients must
        exist for exactly its output rows, and for self/initialize the stock
        buffer must already have the output's shape (the scalar path below
        re-seeds a missing or misshapen one)."""
        if self.gm1_rows is None:
            return False
        if self._uniform and not ops.uses_hip(eps):
            # no kernel for this tensor (CPU, f32, forced eager) and every
            # row holds the scalars: the scalar chain below IS the step, as
            # it always was; ops.rcfg_apply's torch fallback is for rows
            # that differ
            return False
        rows = self.gm1_rows.numel()
        if self.cfg_type == "full":
            return eps.shape[0] == 2 * rows
        return (eps.shape[0] == rows + extra_rows
                and self.stock_noise is not None
                and self.stock_noise.shape == (rows, *eps.shape[1:])
                and self.stock_noise.dtype == eps.dtype)

    def apply(self, eps: torch.Tensor, frame_buffer_size: int) -> torch.Tensor:
        """eps is the raw UNet output batch.

        For cfg_type "full" the batch is [uncond | cond] stacked on dim 0;
        for "initialize" the first frame_buffer_size rows are the uncond
        seed pass; otherwise eps is the conditional batch.
        Returns the guided eps with the stream-batch row count.
        """
        if self.active and self._per_row(
                eps, frame_buffer_size if self.cfg_type == "initialize" else 0):
            if self.cfg_type == "full":
                return ops.rcfg_apply("full", eps, frame_buffer_size,
                                      g=self.g_rows)
            return ops.rcfg_apply(self.cfg_type, eps, frame_buffer_size,
                                  gm1=self.gm1_rows, delta=self.delta_rows,
                                  stock=self.stock_noise)

        # scalar path (no per-row tensors: reset() has not run on this batch
        # shape); a runtime instance at g <= 1 guides with the effective 1.0
        g = max(self.guidance_scale, 1.0)
        if self.cfg_type == "full" and self.active:
            half = eps.shape[0] // 2
            eps_u, eps_c = eps[:half], eps[half:]
            return eps_u + g * (eps_c - eps_u)

        if self.cfg_type == "initialize" and self.active:
            seed, eps_c = eps[:frame_buffer_size], eps[frame_buffer_size:]
            if self.stock_noise is None or self.stock_noise.shape != eps_c.shape:
                self.stock_noise = eps_c.detach().clone()
            # seed pass overwrites the first stage's stock rows (in place:
            # graph-capturable, stable address)
            self.stock_noise[:frame_buffer_size].copy_(seed)
            out = eps_c + (g - 1.0) * (eps_c - self.delta * self.stock_noise)
            self._shift_stock(eps_c, frame_buffer_size)
            return out

        if self.cfg_type == "self" and self.active:
            if self.stock_noise is None or self.stock_noise.shape != eps.shape:
                self.stock_noise = eps.detach().clone()
            out = eps + (g - 1.0) * (eps - self.delta * self.stock_noise)
            self._shift_stock(eps, frame_buffer_size)
            return out

        if self.cfg_type == "initialize":
            # inactive guidance: drop the seed rows
            return eps[frame_buffer_size:]
        return eps

    def _shift_stock(self, eps_c: torch.Tensor, fbs: int) -> None:
        """Stage i's conditional eps becomes stage i+1's negative residual.

        In-place (copy_) into the stable stock buffer so the update is
        hipGraph-capturable: the graph reads and writes the SAME address
        every replay (SURVEY.md §7 hard part #2)."""
        shifted = torch.cat([eps_c[:fbs], eps_c[:-fbs]], dim=0)
        self.stock_noise.copy_(shifted)
