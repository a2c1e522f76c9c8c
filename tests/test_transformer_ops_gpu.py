"""The kernels inside every transformer block (attention, LayerNorm, GEGLU,
the vec8 elementwise family, plus the GroupNorm variance clamp) against
float64 references at the shapes and values where kernels go wrong.

References, case lists, bounds and the constants in them live in
_xfmr_ref.py; the constants are measured from references on the CPU
(test_transformer_ops_cpu.py), never from a kernel's output. Each test prints
its figure before it asserts.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _xfmr_ref as R
from ai_rtc_agent_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ext():
    return ops.hip_ext()


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------

def run_attention(case: R.AttnCase) -> float:
    q, k, v = R.attn_inputs(case, DEV)
    if case.layout == "wrapper":
        got = ops.attention(q, k, v, case.h)      # pads d, true-dim scale
    else:
        got = ext().attention_bhlc(q, k, v, case.h, case.scale)
    assert got.shape == q.shape and got.dtype == torch.float16
    assert torch.isfinite(got).all()
    o, A = R.attn_reference(case.name)
    return R.attn_ratio(got, o, A)


@pytest.mark.parametrize("name", [c.name for c in R.ATTN_CASES])
def test_attention_vs_f64(name):
    ratio = run_attention(R.attn_case(name))
    print(f"{name}: |got-o| / (2^-11 (A+|o|)) = {ratio:.3f} (bound {R.ATTN_C})")
    assert ratio <= R.ATTN_C


def test_attention_kt128_forced_in_a_fresh_process():
    """AIRTC_ATTN_KVT is read once per process: a child runs the Lk=130 case
    (one full 128-key tile and a ragged 2) with the switch set."""
    # the child runs this file as a script, without conftest.py's sys.path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.pathsep.join(p for p in (root, os.environ.get("PYTHONPATH")) if p)
    env = dict(os.environ, AIRTC_ATTN_KVT="128", PYTHONPATH=path)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--forced"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    ratios = json.loads(p.stdout.strip().splitlines()[-1])
    print(ratios)
    assert set(ratios) == {c.name for c in R.ATTN_FORCED}
    for name, ratio in ratios.items():
        assert ratio <= R.ATTN_C, name


def test_attention_bhlc_refuses_what_the_kernel_cannot_read():
    """Every refusal comes from the binding's checks, in front of the launch."""
    B, L, H, d = 2, 64, 2, 64
    C = H * d
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, L, C, generator=g).half().to(DEV) for _ in range(3))
    scale = 1.0 / math.sqrt(d)
    f = ext().attention_bhlc
    f(q, k, v, H, scale)  # the well-formed call runs
    with pytest.raises(RuntimeError, match="unit channel stride"):
        f(q.transpose(1, 2).contiguous().transpose(1, 2), k, v, H, scale)
    with pytest.raises(RuntimeError, match="unit channel stride"):
        f(q, k.transpose(1, 2).contiguous().transpose(1, 2),
          v.transpose(1, 2).contiguous().transpose(1, 2), H, scale)
    kv = torch.cat([k, v], dim=-1)
    with pytest.raises(RuntimeError, match="share layout"):
        f(q, k, kv.chunk(2, dim=-1)[1], H, scale)
    # d = 40: not a multiple of 32
    with pytest.raises(RuntimeError, match="head_dim"):
        f(q[..., :80].contiguous(), k[..., :80].contiguous(),
          v[..., :80].contiguous(), 2, scale)
    # row stride C + 4: rows no longer start on 16 bytes
    wide = torch.zeros(B, L, C + 4, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        f(wide[..., :C], k, v, H, scale)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        f(q, wide[..., :C], wide[..., :C], H, scale)
    # an aligned stride but a base 8 bytes into a row
    off = torch.zeros(B, L, C + 8, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="16-byte"):
        f(off[..., 4:C + 4], k, v, H, scale)
    with pytest.raises(RuntimeError, match="float16"):
        f(q.float(), k.float(), v.float(), H, scale)
    torch.cuda.synchronize()


def _module_case(dim, heads, cross, seed):
    from ai_rtc_agent_amd.models.unet import CrossAttention

    g = torch.Generator().manual_seed(seed)
    ctx_dim = 128 if cross else dim
    mod = CrossAttention(dim, ctx_dim, heads)
    for lin in (mod.to_q, mod.to_k, mod.to_v, mod.to_out):
        lin.weight.data = torch.randn(lin.weight.shape, generator=g) / math.sqrt(lin.weight.shape[1])
    mod.to_out.bias.data = torch.randn(dim, generator=g)
    x = torch.randn(2, 64, dim, generator=g).half()
    ctx = torch.randn(2, 77, ctx_dim, generator=g).half() if cross else None
    return mod.half(), x, ctx


@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("dim,heads", [(320, 8), (640, 8)])
def test_cross_attention_module_padded_heads(dim, heads, cross):
    """CrossAttention with head dims 40 and 80 (zero rows padded into the
    weights, chunk() views of the fused projection, the true-dim scale)
    against the module's math at the TRUE head dim, in float64 from the same
    f16 weights on the CPU.

    Tolerance, as in test_linear_epilogue_gpu.py: the error of the plain
    f16 torch path (three F.linear, f32 SDPA at the true head dim, F.linear
    with bias; unpadded weights) against the same reference, plus what the
    module may add to it. Both paths round q, k, v to f16 off the same
    GEMMs and differ in the attention output only: the kernel's is within
    ATTN_C 2^-11 (A + |o|) of exact, the f32 path's within its f16 rounding
    2^-11 |o|. The out projection is linear, so the results differ by at most
    that difference times |W_out|, plus one f16 ulp at the largest magnitude
    for the final rounding landing on the other side.
    """
    mod, x, ctx = _module_case(dim, heads, cross, seed=dim + cross)
    d = dim // heads
    src = x if ctx is None else ctx
    w = {n: getattr(mod, n).weight.detach() for n in ("to_q", "to_k", "to_v", "to_out")}
    bias = mod.to_out.bias.detach()

    # float64, true head dim, CPU weights
    q64 = x.double() @ w["to_q"].double().T
    k64 = src.double() @ w["to_k"].double().T
    v64 = src.double() @ w["to_v"].double().T
    o64, A64 = R.attn_ref64(q64, k64, v64, heads, 1.0 / math.sqrt(d))
    wo = w["to_out"].double()
    ref = o64 @ wo.T + bias.double()

    # the plain f16 torch path on the device
    xd, sd = x.to(DEV), src.to(DEV)
    wd = {n: t.to(DEV) for n, t in w.items()}
    qh, kh, vh = (R.split_heads(F.linear(a, wd[n]), heads).float()
                  for a, n in ((xd, "to_q"), (sd, "to_k"), (sd, "to_v")))
    o16 = R.merge_heads(F.scaled_dot_product_attention(qh, kh, vh)).half()
    old = F.linear(o16, wd["to_out"], bias.to(DEV))

    mod = mod.to(DEV)
    got = mod(xd, None if ctx is None else ctx.to(DEV))
    assert mod.dpad in (64, 96) and mod.dpad != d
    assert got.shape == (2, 64, dim) and torch.isfinite(got).all()

    err_new = (got.double().cpu() - ref).abs().max().item()
    err_old = (old.double().cpu() - ref).abs().max().item()
    d_o = R.ATTN_C * R.U16 * (A64 + o64.abs()) + R.U16 * o64.abs()
    ulp = 2.0 ** (math.floor(math.log2(ref.abs().max().item())) - 10)
    extra = (d_o @ wo.abs().T).max().item() + ulp
    print(f"dim={dim} cross={cross}: err_new={err_new:.3e} err_old={err_old:.3e} "
          f"extra={extra:.3e} max|ref|={ref.abs().max().item():.3f}")
    assert err_new <= err_old + extra


# ---------------------------------------------------------------------------
# layer norm
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("c,rows,dist", R.LN_CASES)
def test_layer_norm_vs_f64(c, rows, dist):
    x, gamma, beta = R.ln_inputs(c, rows, dist)
    ref, slack, declared = R.ln_reference(c, rows, dist)
    got = ops.layer_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV), R.LN_EPS)
    assert got.shape == x.shape and got.dtype == torch.float16
    got = got.double().cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    r1 = (err / R.ln_bound(ref, slack)).max().item()
    r2 = (err / R.ln_bound_declared(ref, declared)).max().item()
    print(f"C={c} rows={rows} {dist}: err/bound = {r1:.3e} (measured k), "
          f"{r2:.3f} (derived)")
    assert r1 <= 1.0
    assert r2 <= 1.0
    if dist == "const-row":
        # a constant row is beta, whatever its value
        r = R.ln_const_row(rows)
        assert torch.equal(got[r], beta.half().double())


@pytest.mark.parametrize("dist", ["mean64", "const-row"])
def test_layer_norm_row_wider_than_the_register_path(dist):
    """C > 2048 no longer fits four vectors per lane: the kernel re-reads the
    row for each sweep. Same bounds."""
    c, rows = 2056, 5
    x, gamma, beta = R.ln_inputs(c, rows, dist)
    ref, slack, declared = R.ln_reference(c, rows, dist)
    got = ops.layer_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV), R.LN_EPS).double().cpu()
    err = (got - ref).abs()
    assert torch.isfinite(got).all()
    assert (err <= R.ln_bound(ref, slack)).all()
    assert (err <= R.ln_bound_declared(ref, declared)).all()


def test_layer_norm_width_not_a_multiple_of_8():
    """The wrapper routes C % 8 != 0 to the torch path; the binding refuses
    it instead of mis-addressing."""
    g = torch.Generator().manual_seed(77)
    x = torch.randn(3, 5, 77, generator=g).half()
    gamma, beta = torch.randn(77, generator=g), torch.randn(77, generator=g)
    got = ops.layer_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV))
    assert got.shape == x.shape and got.dtype == torch.float16
    x64 = x.double()
    ref = F.layer_norm(x64, (77,), gamma.double(), beta.double())
    z = (x64 - x64.mean(-1, keepdim=True)).abs() / \
        (x64.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    slack = z * gamma.double().abs() + beta.double().abs()
    assert ((got.double().cpu() - ref).abs() <= R.ln_bound(ref, slack)).all()
    with pytest.raises(RuntimeError, match="8 channels"):
        ext().layer_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-5)


# ---------------------------------------------------------------------------
# group norm: the variance clamp
# ---------------------------------------------------------------------------

GN_CONST = 100.125


def _gn_case():
    g = torch.Generator().manual_seed(64)
    x = torch.randn(2, 8, 8, 64, generator=g)
    x[1, :, :, 6:8] = GN_CONST          # batch 1, group 3 of 32 (Cg = 2)
    gamma = torch.randn(64, generator=g) * 0.5 + 1.0
    beta = torch.randn(64, generator=g)
    return x.half(), gamma, beta


@pytest.mark.parametrize("silu", [False, True])
def test_group_norm_constant_group(silu):
    x, gamma, beta = _gn_case()
    got = ops.group_norm_silu_nhwc(x.to(DEV), 32, gamma.to(DEV), beta.to(DEV),
                                   1e-5, silu=silu).double().cpu()
    assert torch.isfinite(got).all()
    ref = F.group_norm(x.double().permute(0, 3, 1, 2), 32, gamma.double(),
                       beta.double(), 1e-5).permute(0, 2, 3, 1)
    if silu:
        ref = ref * torch.sigmoid(ref)
    # Worst-case f32 rounding of the kernel's one-pass statistics, u = 2^-24,
    # n = 128 values per group, in units of sigma (derivation in the style of
    # _xfmr_ref.ln_reference). Recursive sums err by at most n*u of the sum of
    # magnitudes: the mean by n*u*mean|x| <= n*u*(|mu| + sigma), E[x^2] by
    # n*u*(mu^2 + sigma^2). On these groups |mu| <= sigma (N(0,1) draws; the
    # constant group has every sum exact), so the mean moves by <= 2nu sigma
    # and var = E[x^2] - mean^2 by <= 2nu sigma^2 + 2|mu|*2nu sigma <= 6nu
    # sigma^2, i.e. sigma by 3nu relative: |dz| <= 2nu + 3nu|z| <= 4nu(1+|z|)
    # with the constant roundings of the apply. SiLU's slope is below 1.1.
    # Then one f16 rounding (2^-25: half a subnormal step).
    n, u = 128, 2.0 ** -24
    z = F.group_norm(x.double().permute(0, 3, 1, 2), 32, None, None,
                     1e-5).permute(0, 2, 3, 1).abs()
    bound = R.U16 * ref.abs() + 2.0 ** -25 + \
        1.1 * 4 * n * u * ((1 + z) * gamma.double().abs() + beta.double().abs())
    err = (got - ref).abs()
    print(f"silu={silu}: max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    # the constant group: (x - mean) is exactly 0, so the result is beta
    want = beta[6:8].double()
    if silu:
        want = want * torch.sigmoid(want)
    assert R.within_ulp(got[1, :, :, 6:8].half(),
                        want.expand(8, 8, 2).contiguous()).all()


def test_group_norm_coeffs_constant_group():
    x, gamma, beta = _gn_case()
    co = ops.group_norm_coeffs(x.to(DEV), 32, gamma.to(DEV), beta.to(DEV), 1e-5)
    assert co.shape == (2, 64, 2) and co.dtype == torch.float32
    co = co.double().cpu()
    assert torch.isfinite(co).all()
    # float64 from the f16 input: s = gamma * rstd, t = beta - mean * s
    xg = x.double().reshape(2, 64, 32, 2)
    mean = xg.mean(dim=(1, 3)).repeat_interleave(2, dim=1)           # (B, C)
    rstd = (xg.var(dim=(1, 3), unbiased=False) + 1e-5).rsqrt().repeat_interleave(2, dim=1)
    s_ref = gamma.double()[None] * rstd
    t_ref = beta.double()[None] - mean * s_ref
    # from the derivation in the test above: rstd within 3nu relative, the
    # mean within 2nu of a sigma (exact on the constant group); 4nu covers
    # each with the roundings of the two products
    n, u = 128, 2.0 ** -24
    s_bound = 4 * n * u * s_ref.abs()
    t_bound = 4 * n * u * (s_ref.abs() * (mean.abs() + 1) + beta.double().abs()[None])
    # the constant group has sigma^2 = 0: rstd = 1/sqrt(eps), mean exact
    assert (co[..., 0] - s_ref).abs().le(s_bound).all()
    assert (co[..., 1] - t_ref).abs().le(t_bound).all()
    s, t = co[1, 6:8, 0], co[1, 6:8, 1]
    # x*s + t gives beta back up to the f32 rounding of mean*s
    assert ((GN_CONST * s + t - beta[6:8].double()).abs()
            <= 2 * u * (GN_CONST * s).abs()).all()


# ---------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------

def _report(name, ok):
    bad = (~ok).sum().item()
    print(f"{name}: {bad} of {ok.numel()} elements outside the bound")
    return bad == 0


@pytest.mark.parametrize("numel", R.EW_NUMELS)
def test_silu_vs_f64(numel):
    x = R.ew_input(numel, 21)
    got = ops.silu(x.to(DEV)).cpu()
    assert _report(f"silu n={numel}", R.within_ulp(got, R.silu_ref64(x)))


@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_SILU, ops.ACT_RELU])
@pytest.mark.parametrize("numel", R.EW_NUMELS)
def test_add_act_vs_f64(numel, act):
    a = R.ew_input(numel, 31)
    b = R.ew_input(numel, 32, shift=2)
    got = ops.add_act(a.to(DEV), b.to(DEV), act).cpu()
    assert _report(f"add_act n={numel} act={act}",
                   R.within_ulp(got, R.add_act_ref64(a, b, act)))


def test_add_act_refuses_mismatched_operands():
    a = torch.zeros(64, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="elements"):
        ext().add_act(a, a[:32].contiguous(), 0)
    with pytest.raises(RuntimeError, match="elements"):
        ext().add_act(a[:32].contiguous(), a, 0)
    with pytest.raises(RuntimeError, match="float16"):
        ext().add_act(a, a.float(), 0)
    with pytest.raises(RuntimeError, match="float16"):
        ext().add_act(a.float(), a.float(), 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows,inner", R.GEGLU_SHAPES)
def test_geglu_vs_f64(rows, inner):
    x = R.geglu_inputs(rows, inner)
    ref, ab = R.geglu_ref64(x)
    got = ops.geglu(x.to(DEV)).cpu()
    assert got.shape == (rows, inner)
    assert _report(f"geglu {rows}x{inner}",
                   R.within_ulp(got, ref, ab * R.GEGLU_K * 2.0 ** -23))


def test_geglu_inner_not_a_multiple_of_8():
    x = R.ew_input(3 * 2 * 12, 41).view(3, 24)     # inner = 12
    ref, ab = R.geglu_ref64(x)
    got = ops.geglu(x.to(DEV)).cpu()
    assert got.shape == (3, 12)
    assert R.within_ulp(got, ref, ab * R.GEGLU_K * 2.0 ** -23).all()
    with pytest.raises(RuntimeError, match="8 channels"):
        ext().geglu(x.to(DEV))


@pytest.mark.parametrize("shape", R.U8_SHAPES)
def test_preprocess_from_u8_vs_f64(shape):
    u8 = R.u8_frame(shape)
    got = ops.preprocess_from_u8(u8.to(DEV), torch.float16).cpu()
    assert got.shape == shape and got.dtype == torch.float16
    ok = R.within_ulp(got, R.preprocess_ref64(u8))
    tail = math.prod(shape) % 8
    print(f"preprocess {shape}: tail of {tail}, last values {got.flatten()[-8:].tolist()}")
    assert _report(f"preprocess {shape}", ok)


@pytest.mark.parametrize("shape", R.U8_SHAPES)
def test_postprocess_to_u8_vs_f64(shape):
    x = R.post_ramp(shape)
    got = ops.postprocess_to_u8(x.to(DEV)).cpu()
    assert got.shape == shape and got.dtype == torch.uint8
    diff = got != R.postprocess_ref(x)
    tie = R.postprocess_f32_tie(x)
    print(f"postprocess {shape}: {diff.sum().item()} differ, "
          f"{(diff & ~tie).sum().item()} of them not f32 ties")
    assert not (diff & ~tie).any()


@pytest.mark.parametrize("c", [8, 24, 12])
def test_upsample_nearest2x_exact(c):
    g = torch.Generator().manual_seed(c)
    x = torch.randn(2, 5, 7, c, generator=g).half()
    got = ops.upsample_nearest2x_nhwc(x.to(DEV)).cpu()
    ref = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(got, ref)


if __name__ == "__main__":
    # child of test_attention_kt128_forced_in_a_fresh_process
    assert sys.argv[1:] == ["--forced"] and os.environ.get("AIRTC_ATTN_KVT") == "128"
    print(json.dumps({c.name: run_attention(c) for c in R.ATTN_FORCED}))
