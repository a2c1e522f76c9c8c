"""Shared references for the per-slot LoRA tests: the float64 evaluation of
ops.lora_delta_ with its derived error bound, exact-integer operands for the
fragment-layout test, and the adapter files the loader / engine tests use.

Nothing here is tuned: every bound is a sum of worst-case rounding terms
whose magnitudes come from the float64 evaluation.
"""
from __future__ import annotations

import torch

U16 = 2.0 ** -11  # f16 unit roundoff
U32 = 2.0 ** -24  # f32 unit roundoff


def gamma(n: int, u: float = U32) -> float:
    """First-order bound on n chained roundings of unit roundoff u."""
    return n * u


def lora_delta_f64(y, x, A, B, row_adapter, row_scale, col_offset=0):
    """float64 evaluation of the op on the inputs' exact values.

    Returns (result, mags): result is y's shape in float64; mags holds, for
    the written column range, the magnitudes the bound needs:
      t      (Bt, L, R)  the exact intermediate x.A^T
      abs_t  (Bt, L, R)  sum_k |x||A|
      tb     (Bt, L, N)  sum_r |t_r||B_nr|
      atb    (Bt, L, N)  sum_r (sum_k |x||A|)_r |B_nr|
      d      (Bt, L, N)  the exact second product (before the scale)
    Rows with row_adapter < 0 have zero magnitudes and an unchanged result.
    """
    Bt = x.shape[0]
    N = B.shape[1]
    n = A.shape[0]
    xd, yd = x.double().cpu(), y.double().cpu()
    Ad, Bd = A.double().cpu(), B.double().cpu()
    ra = row_adapter.cpu()
    s = row_scale.double().cpu()
    on = (ra >= 0) & (ra < n)
    idx = ra.clamp(0, n - 1).long()
    Ab, Bb = Ad[idx], Bd[idx]
    t = torch.bmm(xd, Ab.transpose(1, 2))
    abs_t = torch.bmm(xd.abs(), Ab.abs().transpose(1, 2))
    d = torch.bmm(t, Bb.transpose(1, 2))
    tb = torch.bmm(t.abs(), Bb.abs().transpose(1, 2))
    atb = torch.bmm(abs_t, Bb.abs().transpose(1, 2))
    m = on.view(-1, 1, 1).double()
    out = yd.clone()
    out[:, :, col_offset:col_offset + N] += m * s.view(-1, 1, 1) * d
    mags = {"t": t * m, "abs_t": abs_t * m, "tb": tb * m, "atb": atb * m,
            "d": d * m}
    return out, mags


def lora_delta_bound(ref, mags, row_scale, K, R, N, col_offset=0, u=U16):
    """Per-element bound on |op - ref| for storage roundoff u (f16: 2^-11,
    f32: 2^-24) and f32 accumulation, y's shape. Outside the written
    columns, and on rows without an adapter, it is exactly zero.

      u |ref|                          the one final rounding
      |s| sum_r u |t_r| |B_nr|         the intermediate's rounding to storage
      |s| gamma_K sum_r (sum_k|x||A|)_r |B_nr|   first product, f32 sums
      |s| gamma_R (1+u) sum_r |t_r| |B_nr|       second product, f32 sums
      gamma_2 (|y| + |s d|)            scale multiply and the add, in f32
    """
    s = row_scale.double().cpu().abs().view(-1, 1, 1)
    sl = slice(col_offset, col_offset + N)
    active = (mags["abs_t"].sum(dim=(1, 2)) > 0).view(-1, 1, 1).double()
    bound = torch.zeros_like(ref)
    sd = s * mags["d"].abs()
    y_in = ref[:, :, sl].abs() + sd  # |y| <= |ref| + |s d|
    bound[:, :, sl] = active * (
        u * ref[:, :, sl].abs()
        + s * u * mags["tb"]
        + s * gamma(K) * mags["atb"]
        + s * gamma(R) * (1 + u) * mags["tb"]
        + gamma(2) * (y_in + sd)
    )
    return bound


# -- exact-integer operands ---------------------------------------------------

def int_case(Bt, L, K, N, Ny, R, n_adapters=3, device="cpu",
             dtype=torch.float16):
    """x, A, B in {-1, 0, 1} on non-symmetric patterns, y integers of
    magnitude <= 512. A's rows hold 8 non-zeros, B's rows 4, at positions
    that move with the row, so |t| <= 8 and |y + 2 (t.B^T)| <= 576: every
    intermediate and result is an integer far below 2048 and the f16 answer
    is exact for every K and R of the test. Any difference is a transposed
    or permuted fragment."""
    def grid(*shape):
        return torch.meshgrid(*[torch.arange(s) for s in shape], indexing="ij")

    b, l, k = grid(Bt, L, K)
    x = (b * 7 + l * 3 + k * 5 + (l * k) % 11) % 3 - 1
    a, r, k = grid(n_adapters, R, K)
    A = torch.where((k + 3 * r + a) % (K // 8) == 0,
                    ((k * r + k // 3 + a) % 2) * 2 - 1, 0)
    a, n, r = grid(n_adapters, N, R)
    Bm = torch.where((r + 5 * n + a) % (R // 4) == 0,
                     ((r // 2 + n * r + n + a) % 2) * 2 - 1, 0)
    b, l, c = grid(Bt, L, Ny)
    y = (b * 131 + l * 17 + c * 29) % 1025 - 512
    return tuple(t.to(dtype).to(device).contiguous() for t in (x, y, A, Bm))


# -- adapter files ------------------------------------------------------------

def attention_lora(unet, rank=4, seed=0, std=0.05, only=None):
    """An own-path adapter (as make_random_lora writes them) over every
    Linear of every SpatialTransformer: attn1, attn2 (to_k / to_v included),
    ff and the Linear proj_in / proj_out. `only` keeps the module paths that
    contain it."""
    from ai_rtc_agent_amd.models.unet import Linear, SpatialTransformer

    g = torch.Generator().manual_seed(seed)
    sd = {}
    for tname, t in unet.named_modules():
        if not isinstance(t, SpatialTransformer):
            continue
        for name, m in t.named_modules():
            if not isinstance(m, Linear):
                continue
            path = f"{tname}.{name}"
            if only is not None and only not in path:
                continue
            o, i = m.weight.shape
            sd[f"{path}.lora_down.weight"] = torch.randn(rank, i, generator=g) * std
            sd[f"{path}.lora_up.weight"] = torch.randn(o, rank, generator=g) * std
            sd[f"{path}.alpha"] = torch.tensor(float(rank) / 2)
    return sd
