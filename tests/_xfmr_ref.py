"""Shared helpers of test_transformer_ops_cpu.py / test_transformer_ops_gpu.py:
float64 references, the attention emulator, the f16 ulp distance and the case
lists. Neither a conftest nor a test module.

How the op tests bound error (same text, with the reasoning, in
docs/kernels.md, "How the op tests bound error"):

attention   |got - o| <= ATTN_C * 2^-11 * (A + |o|), o = softmax(S)·V and
            A = softmax(S)·|V| in float64 from the f16 inputs. The kernel
            rounds P to f16 before PV and the result to f16; everything else
            is f32. ATTN_C is NOT taken from the kernel: `attn_emulate`
            below performs the declared arithmetic in torch, the CPU test
            measures max |emu - o| / (2^-11 (A + |o|)) over ATTN_CASES and
            ATTN_C is twice that (hardware exp2, MFMA accumulation order).
            Measured maximum 0.855 (case tmpl-d64-peaked), ATTN_C = 1.71.
layer norm  |got - ref| <= 2^-11 |ref| + LN_K * 2^-24 * (|x-mu|/sigma*|gamma|
            + |beta|), ref = F.layer_norm in float64. LN_K is twice the
            largest such ratio of torch's own f32 CPU LayerNorm (before any
            f16 rounding) over LN_CASES. Measured maximum 195 070 at
            (C=320, rows=308, mean 64): torch's vectorised f32 path is not
            two-pass at rows > 1 and loses the variance of an offset row
            itself, so LN_K = 390 140 is loose there. `ln_bound_declared`
            is therefore asserted as well: the worst-case rounding analysis
            of the arithmetic the kernel declares (deviations from the row's
            first element, which f32 holds exactly for values of similar
            magnitude and to one rounding otherwise; mean of those; centred
            sum of squares; variance clamped at 0), no measured constant:
            2^-11 |ref| + 2^-25 + 2^-24 * ((C+8)*(zp+2)*(1+|z|)*|gamma|
                                           + 2*(|z||gamma| + |beta|)),
            z = (x-mu)/sigma, zp = |x[0]-mu|/sigma; 2^-25 is half the f16
            subnormal spacing.
elementwise reference in float64 rounded once to f16; distance <= 1 f16 ulp
            (f32 compute + one rounding cannot be further from the correctly
            rounded value). GEGLU's negative tail cancels in 1 + erf, so its
            reference may first move by |a|*|b|*GEGLU_K*2^-23; GEGLU_K is
            twice the largest |f32 - f64| / (|a||b| 2^-23) of torch's f32 CPU
            GEGLU on the same inputs. Measured maximum 2.052 (rows=1,
            inner=1288), GEGLU_K = 4.11.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

U16 = 2.0 ** -11   # f16 unit roundoff
LOG2E = 1.44269504088896340736

# measured by test_transformer_ops_cpu.py (which fails if they go stale)
ATTN_EMU_MAX = 0.855
ATTN_C = 1.71
LN_F32_MAX = 195070.0
LN_K = 390140.0
GEGLU_F32_MAX = 2.052
GEGLU_K = 4.11


# ---------------------------------------------------------------------------
# f16 ulp distance
# ---------------------------------------------------------------------------

def f16_ord(x: torch.Tensor) -> torch.Tensor:
    """f16 -> int32 that steps by one per representable value: -0 and +0
    both map to 0, +-inf to +-0x7c00. NaN is the caller's business."""
    assert x.dtype == torch.float16
    bits = x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = bits & 0x7FFF
    return torch.where(bits >= 0x8000, -mag, mag)


def f16_ulp_dist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Number of representable f16 values between a and b (0 = equal)."""
    return (f16_ord(a) - f16_ord(b)).abs()


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------

REGIMES = ("normal", "peaked", "offset")


@dataclass(frozen=True)
class AttnCase:
    name: str
    d: int              # true head dim
    lq: int
    lk: int
    regime: str
    b: int = 2
    h: int = 2
    layout: str = "plain"   # plain | qkv | kv | kv_expand | wrapper
    kt: int = 0             # 0 = the dispatcher's choice

    @property
    def tile(self) -> int:
        """kv tile the dispatcher runs this case at."""
        if self.kt:
            return self.kt if self.lk >= 128 else 64
        return 128 if self.lk >= 1024 else 64

    @property
    def scale(self) -> float:
        return 1.0 / math.sqrt(self.d)


def _attn_geometries():
    g = []
    # every template, two ragged tiles, a second workgroup with 6 live rows
    for d in (32, 64, 96, 128, 160):
        g.append(dict(name=f"tmpl-d{d}", d=d, lq=70, lk=77))
    # KT=128 route (auto at Lk >= 1024): ragged last tile of 6 keys, and an
    # exact multiple of 128
    for d in (64, 96, 160):
        g.append(dict(name=f"kt128-d{d}-lk1030", d=d, lq=64, lk=1030, h=1))
    g.append(dict(name="kt128-d64-lk1152", d=64, lq=64, lk=1152, h=1))
    # short and exact tiles
    for lq, lk in ((1, 1), (16, 16), (64, 64), (65, 65), (1, 128), (64, 1),
                   (16, 65), (65, 128)):
        g.append(dict(name=f"edge-lq{lq}-lk{lk}", d=64, lq=lq, lk=lk))
    # the model's layouts
    g.append(dict(name="qkv-d64", d=64, lq=70, lk=70, layout="qkv"))
    g.append(dict(name="kv-d64", d=64, lq=64, lk=77, layout="kv"))
    g.append(dict(name="kv-d96", d=96, lq=64, lk=77, layout="kv"))
    g.append(dict(name="kvexpand-d64", d=64, lq=64, lk=77, layout="kv_expand"))
    # padded heads through the ops.attention wrapper
    g.append(dict(name="wrap-d40", d=40, lq=70, lk=77, layout="wrapper"))
    g.append(dict(name="wrap-d80", d=80, lq=70, lk=77, layout="wrapper"))
    return g


ATTN_CASES = tuple(
    AttnCase(**{**geo, "name": f"{geo['name']}-{r}"}, regime=r)
    for geo in _attn_geometries() for r in REGIMES)

# KT=128 below Lk=1024: only reachable with AIRTC_ATTN_KVT=128 (cached in a
# static, so a fresh process); tiles of 128 and a ragged 2
ATTN_FORCED = tuple(
    AttnCase(name=f"forced128-lk130-{r}", d=64, lq=70, lk=130, regime=r, kt=128)
    for r in REGIMES)

ATTN_ALL = ATTN_CASES + ATTN_FORCED


def attn_case(name: str) -> AttnCase:
    return next(c for c in ATTN_ALL if c.name == name)


def attn_inputs(case: AttnCase, device="cpu"):
    """Seeded f16 (q, k, v) as (B, L, H*d) tensors in the case's layout: the
    values are drawn on the CPU and do not depend on `device`."""
    g = torch.Generator().manual_seed(7000 + ATTN_ALL.index(case))
    B, H, d, lq, lk = case.b, case.h, case.d, case.lq, case.lk
    C = H * d
    qs = 6.0 if case.regime == "peaked" else 1.0
    vo = 3.0 if case.regime == "offset" else 0.0

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    if case.layout == "qkv":
        t = rn(B, lq, 3 * C)
        t[..., :C] *= qs
        t[..., 2 * C:] += vo
        q, k, v = t.half().to(device).chunk(3, dim=-1)
        return q, k, v
    q = (rn(B, lq, C) * qs).half().to(device)
    if case.layout in ("kv", "kv_expand"):
        kb = 1 if case.layout == "kv_expand" else B
        t = rn(kb, lk, 2 * C)
        t[..., C:] += vo
        t = t.half().to(device)
        if case.layout == "kv_expand":
            t = t.expand(B, lk, 2 * C)
        k, v = t.chunk(2, dim=-1)
        return q, k, v
    k = rn(B, lk, C).half().to(device)
    v = (rn(B, lk, C) + vo).half().to(device)
    return q, k, v


def split_heads(t: torch.Tensor, h: int) -> torch.Tensor:
    b, l, c = t.shape
    return t.reshape(b, l, h, c // h).permute(0, 2, 1, 3)


def merge_heads(t: torch.Tensor) -> torch.Tensor:
    b, h, l, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, l, h * d)


def attn_ref64(q, k, v, h: int, scale: float):
    """float64 softmax attention from the exact f16 inputs. Returns (o, A),
    both (B, Lq, C): o = softmax(S)·V, A = softmax(S)·|V|."""
    qh, kh, vh = (split_heads(t.detach().cpu().double(), h) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    return merge_heads(p @ vh), merge_heads(p @ vh.abs())


def attn_emulate(q, k, v, h: int, scale: float, kt: int) -> torch.Tensor:
    """The kernel's DECLARED arithmetic in torch (attention.hip): f32 logits
    in the base-2 domain, online softmax per kt-wide tile with m starting at
    -1e30, P cast to f16 for the PV product only while l sums the unrounded
    f32 P, f32 accumulation, f16 result."""
    qh, kh, vh = (split_heads(t.detach().cpu().float(), h) for t in (q, k, v))
    scale2 = torch.tensor(scale, dtype=torch.float32) * \
        torch.tensor(LOG2E, dtype=torch.float32)
    s = (qh @ kh.transpose(-1, -2)) * scale2                    # (B,H,Lq,Lk)
    lk = s.shape[-1]
    m = torch.full(s.shape[:-1], -1e30, dtype=torch.float32)
    l = torch.zeros_like(m)
    acc = torch.zeros(*s.shape[:-1], vh.shape[-1], dtype=torch.float32)
    for t0 in range(0, lk, kt):
        st = s[..., t0:t0 + kt]
        mn = torch.maximum(m, st.amax(dim=-1))
        alpha = torch.exp2(m - mn)
        p = torch.exp2(st - mn[..., None])
        l = l * alpha + p.sum(dim=-1)
        acc = acc * alpha[..., None] + p.half().float() @ vh[..., t0:t0 + kt, :]
        m = mn
    return merge_heads((acc * (1.0 / l)[..., None]).half())


@functools.lru_cache(maxsize=None)
def attn_reference(name: str):
    """(o, A) of a case, computed once and shared; callers do not write."""
    case = attn_case(name)
    q, k, v = attn_inputs(case)
    return attn_ref64(q, k, v, case.h, case.scale)


def attn_ratio(got: torch.Tensor, o: torch.Tensor, A: torch.Tensor) -> float:
    """max |got - o| / (2^-11 (A + |o|))."""
    err = (got.detach().cpu().double() - o).abs()
    return (err / (U16 * (A + o.abs()))).max().item()


# ---------------------------------------------------------------------------
# layer norm
# ---------------------------------------------------------------------------

LN_DISTS = ("normal", "mean64", "mean-200", "const-row")
LN_CASES = tuple((c, rows, dist) for c in (8, 320, 520, 2048)
                 for rows in (1, 5, 77 * 4) for dist in LN_DISTS)
LN_EPS = 1e-5
LN_CONST = 100.125  # exact in f16


def ln_const_row(rows: int) -> int:
    return rows // 2


def ln_inputs(c: int, rows: int, dist: str):
    """Seeded (x f16 (rows, C), gamma f32, beta f32) on the CPU."""
    g = torch.Generator().manual_seed(
        9000 + 97 * c + 7 * rows + LN_DISTS.index(dist))
    x = torch.randn(rows, c, generator=g)
    if dist == "mean64":
        x = x * 0.25 + 64.0
    elif dist == "mean-200":
        x = x - 200.0
    elif dist == "const-row":
        x[ln_const_row(rows)] = LN_CONST
    gamma = torch.randn(c, generator=g) * 0.5 + 1.0
    beta = torch.randn(c, generator=g)
    return x.half(), gamma, beta


@functools.lru_cache(maxsize=None)
def ln_reference(c: int, rows: int, dist: str):
    """(ref, slack, declared): F.layer_norm in float64 on the f16 input;
    |x - mu|/sigma*|gamma| + |beta|, the factor of the bound's f32 term; and
    the f32 term of ln_bound_declared, in units of 2^-24."""
    x, gamma, beta = ln_inputs(c, rows, dist)
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    ref = F.layer_norm(x64, (c,), g64, b64, LN_EPS)
    mu = x64.mean(dim=-1, keepdim=True)
    sigma = (x64.var(dim=-1, unbiased=False, keepdim=True) + LN_EPS).sqrt()
    z = (x64 - mu).abs() / sigma
    slack = z * g64.abs() + b64.abs()
    # Worst-case f32 rounding of the declared arithmetic, u = 2^-24, n = C,
    # in units of sigma. d_i = x_i - x_0 is exact when the two are of similar
    # magnitude (exponents within 13), otherwise one f32 rounding, which the
    # +8 below absorbs. The mean of d errs by at
    # most n*u*mean|d| <= n*u*(zp + 1) (mean|x - mu| <= sigma). The centred
    # sum of squares errs by (n+1)*u relative from its own summation and by
    # 2*that mean error from its terms, so sigma by n*u*(zp + 2) relative.
    # Together |dz| <= n*u*(zp + 2)*(1 + |z|). The roundings that do not
    # grow with n (centring, rsqrt at 1 ulp, the two products) are the +8;
    # the affine's own adds are the 2u per term.
    zp = z[:, :1]
    declared = (c + 8.0) * (zp + 2.0) * (1.0 + z) * g64.abs() + 2.0 * slack
    return ref, slack, declared


def ln_f32_ratio(c: int, rows: int, dist: str) -> float:
    """torch's f32 CPU LayerNorm against float64, in units of 2^-24 * slack."""
    x, gamma, beta = ln_inputs(c, rows, dist)
    ref, slack, _ = ln_reference(c, rows, dist)
    y32 = F.layer_norm(x.float(), (c,), gamma, beta, LN_EPS).double()
    return ((y32 - ref).abs() / (2.0 ** -24 * slack)).max().item()


def ln_bound(ref: torch.Tensor, slack: torch.Tensor) -> torch.Tensor:
    return U16 * ref.abs() + LN_K * 2.0 ** -24 * slack


def ln_bound_declared(ref: torch.Tensor, declared: torch.Tensor) -> torch.Tensor:
    return U16 * ref.abs() + 2.0 ** -25 + 2.0 ** -24 * declared


def ln_emulate(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """The LayerNorm kernel's declared arithmetic in f32 torch ops."""
    d = x.float() - x.float()[:, :1]
    c = d - d.mean(dim=-1, keepdim=True)
    var = (c * c).mean(dim=-1, keepdim=True).clamp_min(0.0)
    return (c * torch.rsqrt(var + LN_EPS) * gamma + beta).half()


# ---------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------

EW_EXPLICIT = (0.0, -0.0, 65504.0, -65504.0, 20.0, -20.0, -8.0, 1e-4)
# one grid sweep of the vec8 kernels covers EW_MAX_BLOCKS * EW_BLOCK = 2048 *
# 256 lanes of 8 elements: 8 * 65 537 stays inside it, so the third size is
# the smallest numel that needs a second sweep
EW_SWEEP = 2048 * 256
EW_NUMELS = (8, 8 * 257, 8 * (EW_SWEEP + 1))
GEGLU_SHAPES = tuple((r, i) for r in (1, 3) for i in (8, 24, 1288))


def ew_input(numel: int, seed: int, shift: int = 0) -> torch.Tensor:
    """N(0,1)*4 in f16 with the explicit values written over the head,
    rotated by `shift` so two operands pair different extremes."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(numel, generator=g) * 4.0).half()
    ex = torch.tensor(EW_EXPLICIT[shift:] + EW_EXPLICIT[:shift]).half()
    n = min(numel, ex.numel())
    x[:n] = ex[:n]
    return x


def to_f16_once(x64: torch.Tensor) -> torch.Tensor:
    """float64 -> f16 with a single rounding (overflow goes to inf)."""
    return x64.to(torch.float16)


def silu_ref64(x: torch.Tensor) -> torch.Tensor:
    x64 = x.double()
    return x64 * torch.sigmoid(x64)


def add_act_ref64(a: torch.Tensor, b: torch.Tensor, act: int) -> torch.Tensor:
    y = a.double() + b.double()
    if act == 1:
        return y * torch.sigmoid(y)
    if act == 2:
        return torch.relu(y)
    return y


def geglu_inputs(rows: int, inner: int) -> torch.Tensor:
    """(rows, 2*inner) f16: the `a` half and the `b` half both carry the
    explicit values, b's rotated."""
    a = ew_input(rows * inner, 300 + rows * 10000 + inner).view(rows, inner)
    b = ew_input(rows * inner, 301 + rows * 10000 + inner, shift=3).view(rows, inner)
    return torch.cat([a, b], dim=-1).contiguous()


def geglu_ref64(x: torch.Tensor):
    """(a * gelu(b) in float64, |a||b|)."""
    a, b = x.double().chunk(2, dim=-1)
    y = a * (0.5 * b * (1.0 + torch.erf(b / math.sqrt(2.0))))
    return y, (a * b).abs()


def geglu_f32_ratio(x: torch.Tensor) -> float:
    """torch's f32 CPU GEGLU against float64 in units of |a||b| 2^-23, over
    the elements where both are finite."""
    ref, ab = geglu_ref64(x)
    a, b = x.float().chunk(2, dim=-1)
    y32 = (a * F.gelu(b)).double()
    err = (y32 - ref).abs()
    ok = torch.isfinite(y32) & torch.isfinite(ref) & (ab > 0)
    return (err[ok] / (ab[ok] * 2.0 ** -23)).max().item()


def within_ulp(got: torch.Tensor, ref64: torch.Tensor,
               slack: torch.Tensor | None = None, ulps: int = 1):
    """Elementwise: is `got` (f16) within `ulps` f16 steps of the once-rounded
    reference, after the reference may have moved by `slack` (absolute)?
    Rounding is monotonic, so that is ord(round(ref - slack)) - ulps <=
    ord(got) <= ord(round(ref + slack)) + ulps."""
    got = got.detach().cpu()
    if slack is None:
        slack = torch.zeros_like(ref64)
    lo = f16_ord(to_f16_once(ref64 - slack)) - ulps
    hi = f16_ord(to_f16_once(ref64 + slack)) + ulps
    o = f16_ord(got)
    return ~torch.isnan(got) & (o >= lo) & (o <= hi)


U8_SHAPES = ((1, 64, 64, 3), (1, 50, 50, 3), (2, 5, 7, 3))


def u8_frame(shape) -> torch.Tensor:
    """u8 frame that holds every byte value (as many distinct ones as it has
    elements when it is smaller than 256, 0 and 255 among them)."""
    n = math.prod(shape)
    g = torch.Generator().manual_seed(500 + n)
    vals = torch.arange(n) % 256
    if n < 256:
        mid = torch.randperm(254, generator=g)[: n - 2] + 1
        vals = torch.cat([torch.tensor([0, 255]), mid])
    vals = vals[torch.randperm(n, generator=g)]
    return vals.to(torch.uint8).view(shape)


def preprocess_ref64(u8: torch.Tensor) -> torch.Tensor:
    return u8.double() / 127.5 - 1.0


def post_ramp(shape) -> torch.Tensor:
    """f16 ramp over [-1.5, 1.5] with the interesting points written over the
    head: the one exact tie of (x+1)*127.5 an f16 can hold (x = 0, 127.5),
    the range ends, the clamp edges, the smallest subnormals (ties in f32
    only: 1 +- 2^-24 rounds to 1) and the f16 values nearest to every
    would-be tie (2n+1)/255 - 1."""
    n = math.prod(shape)
    x = torch.linspace(-1.5, 1.5, n, dtype=torch.float64).half()
    near = (torch.arange(0, 255, dtype=torch.float64) * 2 + 1) / 255.0 - 1.0
    pts = torch.cat([
        torch.tensor([0.0, -0.0, -1.0, 1.0, -1.5, 1.5, 2.0 ** -24, -2.0 ** -24,
                      2.0 ** -14, -2.0 ** -14], dtype=torch.float64),
        near]).half()
    k = min(n // 2, pts.numel())
    x[:k] = pts[:k]
    return x.view(shape)


def postprocess_ref(x: torch.Tensor) -> torch.Tensor:
    """round-half-even((x+1)*127.5) in float64 from the f16 value, clamped."""
    return torch.round((x.double() + 1.0) * 127.5).clamp(0, 255).to(torch.uint8)


def postprocess_f32_tie(x: torch.Tensor) -> torch.Tensor:
    """Where the kernel's f32 arithmetic ((float)x + 1) * 127.5 lands exactly
    on n + 0.5: the only elements allowed to differ from postprocess_ref."""
    f = (x.float() + 1.0) * 127.5
    return (f - torch.floor(f)) == 0.5
