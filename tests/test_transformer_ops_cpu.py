"""CPU half of the transformer-path op tests: the helpers of _xfmr_ref.py are
themselves checked here, and the constants the GPU tests bound error with are
measured here, from references only (never from a kernel's output).

See _xfmr_ref.py's docstring for the bounds.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _xfmr_ref as R
from ai_rtc_agent_amd import ops


# ---------------------------------------------------------------------------
# ulp distance
# ---------------------------------------------------------------------------

def h(*vals):
    return torch.tensor(vals, dtype=torch.float16)


def test_ulp_distance_steps_by_one_over_every_finite_f16():
    bits = torch.arange(0, 0x7C01, dtype=torch.int32)        # +0 .. +inf
    pos = bits.to(torch.int16).view(torch.float16)
    assert torch.equal(R.f16_ord(pos), bits)
    assert torch.equal(R.f16_ord(-pos), -bits)
    assert (R.f16_ulp_dist(pos[1:], pos[:-1]) == 1).all()
    # the ordering is the ordering of the values
    both = torch.cat([-pos.flip(0), pos])
    assert (both.double().diff() >= 0).all()
    assert (R.f16_ord(both).diff() >= 0).all()


def test_ulp_distance_edges():
    assert R.f16_ulp_dist(h(0.0), h(-0.0)).item() == 0
    assert R.f16_ulp_dist(h(2.0 ** -24), h(-2.0 ** -24)).item() == 2
    assert R.f16_ulp_dist(h(65504.0), h(float("inf"))).item() == 1
    assert R.f16_ulp_dist(h(1.0), h(1.0 + 2.0 ** -10)).item() == 1
    assert R.f16_ulp_dist(h(1.0), h(1.0 - 2.0 ** -11)).item() == 1
    assert R.f16_ulp_dist(h(-3.0), h(-3.0)).item() == 0


def test_within_ulp():
    ref = torch.tensor([1.0, 1.0, 1.0, 70000.0, 0.0], dtype=torch.float64)
    got = h(1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9, float("nan"), float("inf"), -0.0)
    assert R.within_ulp(got, ref).tolist() == [True, False, False, True, True]
    # slack moves the reference before the rounding
    assert R.within_ulp(h(1.0 + 2.0 ** -9), ref[:1],
                        slack=torch.tensor([2.0 ** -10], dtype=torch.float64)).all()


# ---------------------------------------------------------------------------
# attention: the emulator sets ATTN_C
# ---------------------------------------------------------------------------

def test_attention_case_list_covers_the_issue():
    names = {c.name for c in R.ATTN_ALL}
    assert len(names) == len(R.ATTN_ALL)
    geos = {(c.d, c.lq, c.lk, c.layout) for c in R.ATTN_CASES}
    for d in (32, 64, 96, 128, 160):
        assert (d, 70, 77, "plain") in geos
    for d in (64, 96, 160):
        assert (d, 64, 1030, "plain") in geos
    assert (64, 64, 1152, "plain") in geos
    assert {c.lk for c in R.ATTN_CASES if c.name.startswith("edge")} == {1, 16, 64, 65, 128}
    assert {c.lq for c in R.ATTN_CASES if c.name.startswith("edge")} == {1, 16, 64, 65}
    assert {c.layout for c in R.ATTN_CASES} == {"plain", "qkv", "kv", "kv_expand", "wrapper"}
    # three regimes on every geometry
    for c in R.ATTN_ALL:
        stem = c.name.rsplit("-", 1)[0]
        assert {f"{stem}-{r}" for r in R.REGIMES} <= names
    assert all(c.tile == 128 for c in R.ATTN_ALL if c.lk >= 1024 or c.kt == 128)
    assert all(c.tile == 64 for c in R.ATTN_CASES if c.lk < 1024)


def test_attention_inputs_have_the_model_layouts():
    q, k, v = R.attn_inputs(R.attn_case("qkv-d64-normal"))
    assert q.stride(1) == 3 * q.shape[2] and k.storage_offset() == q.shape[2]
    assert v.storage_offset() == 2 * q.shape[2] and not k.is_contiguous()
    q, k, v = R.attn_inputs(R.attn_case("kv-d96-offset"))
    assert k.stride(1) == 2 * k.shape[2] and v.storage_offset() == k.shape[2]
    q, k, v = R.attn_inputs(R.attn_case("kvexpand-d64-peaked"))
    assert k.stride(0) == 0 and v.stride(0) == 0 and k.shape[0] == 2
    # the regimes do what they say
    _, _, v = R.attn_inputs(R.attn_case("tmpl-d64-offset"))
    assert abs(v.float().mean().item() - 3.0) < 0.05
    case = R.attn_case("tmpl-d64-peaked")
    q, k, _ = R.attn_inputs(case)
    s = R.split_heads(q.double(), 2) @ R.split_heads(k.double(), 2).transpose(-1, -2)
    assert 15.0 < (s * case.scale).abs().max().item() < 45.0


def test_attention_reference_matches_f64_sdpa():
    case = R.attn_case("tmpl-d96-offset")
    q, k, v = R.attn_inputs(case)
    o, A = R.attn_reference(case.name)
    qh, kh, vh = (R.split_heads(t.double(), case.h) for t in (q, k, v))
    sd = F.scaled_dot_product_attention(qh, kh, vh, scale=case.scale)
    assert torch.allclose(o, R.merge_heads(sd), rtol=1e-12, atol=1e-13)
    assert (A >= o.abs() - 1e-12).all()


@pytest.fixture(scope="module")
def emulator_ratios():
    out = {}
    for c in R.ATTN_ALL:
        q, k, v = R.attn_inputs(c)
        o, A = R.attn_reference(c.name)
        out[c.name] = R.attn_ratio(R.attn_emulate(q, k, v, c.h, c.scale, c.tile), o, A)
    return out


def test_attention_emulator_sets_the_constant(emulator_ratios):
    worst = max(emulator_ratios, key=emulator_ratios.get)
    print(f"emulator max ratio {emulator_ratios[worst]:.4f} at {worst}; "
          f"min {min(emulator_ratios.values()):.4f}")
    # the recorded figures are the measured ones, and C is twice the maximum
    assert abs(emulator_ratios[worst] - R.ATTN_EMU_MAX) < 5e-3
    assert R.ATTN_C == pytest.approx(2 * R.ATTN_EMU_MAX, abs=5e-3)


@pytest.mark.parametrize("name", [c.name for c in R.ATTN_ALL])
def test_attention_emulator_under_half_the_bound(name, emulator_ratios):
    """The case list cannot drift past the bound unnoticed."""
    assert emulator_ratios[name] <= R.ATTN_C / 2


def test_attention_emulator_sees_a_wrong_kernel():
    """The bound is tight enough for the failures it is there for: a dropped
    kv tile, a stale l, masked columns leaking into the sum."""
    for name in ("kt128-d64-lk1030-normal", "kt128-d64-lk1030-offset",
                 "tmpl-d64-normal", "tmpl-d64-offset"):
        c = R.attn_case(name)
        q, k, v = R.attn_inputs(c)
        o, A = R.attn_reference(name)
        # last (ragged) tile dropped
        cut = (c.lk - 1) // c.tile * c.tile
        bad = R.attn_emulate(q, k[:, :cut], v[:, :cut], c.h, c.scale, c.tile)
        assert R.attn_ratio(bad, o, A) > R.ATTN_C, name
        # one masked column (a copy of the last key, as the kernel stages it)
        # leaking into the sum
        kk = torch.cat([k, k[:, -1:]], dim=1)
        vv = torch.cat([v, v[:, -1:]], dim=1)
        bad = R.attn_emulate(q, kk, vv, c.h, c.scale, c.tile)
        assert R.attn_ratio(bad, o, A) > R.ATTN_C, name
    # a stale l is a pure scale error: only V's offset makes it visible
    o, A = R.attn_reference("kt128-d64-lk1030-offset")
    assert R.attn_ratio((o * (1 + 4 * R.U16)).half(), o, A) > R.ATTN_C


def test_ops_attention_cpu_path_meets_the_bound():
    """The project's own CPU path (f32 SDPA) against the same reference."""
    for name in ("wrap-d40-peaked", "wrap-d80-offset", "tmpl-d64-normal"):
        c = R.attn_case(name)
        q, k, v = R.attn_inputs(c)
        o, A = R.attn_reference(name)
        got = ops.attention(q, k, v, c.h, scale=c.scale)
        assert R.attn_ratio(got, o, A) <= R.ATTN_C


# ---------------------------------------------------------------------------
# layer norm: torch's f32 path sets LN_K
# ---------------------------------------------------------------------------

def test_layer_norm_constant_is_the_measured_one():
    ratios = {case: R.ln_f32_ratio(*case) for case in R.LN_CASES}
    worst = max(ratios, key=ratios.get)
    print(f"torch f32 layer_norm max ratio {ratios[worst]:.1f} at {worst}")
    assert ratios[worst] == pytest.approx(R.LN_F32_MAX, rel=2e-2)
    assert R.LN_K == pytest.approx(2 * R.LN_F32_MAX, rel=1e-3)


@pytest.mark.parametrize("c,rows,dist", R.LN_CASES)
def test_layer_norm_declared_arithmetic_meets_both_bounds(c, rows, dist):
    """ln_emulate is the kernel's arithmetic in f32 torch ops: it must sit
    inside the measured bound and inside the derived one, or the derivation
    is wrong."""
    x, gamma, beta = R.ln_inputs(c, rows, dist)
    ref, slack, declared = R.ln_reference(c, rows, dist)
    err = (R.ln_emulate(x, gamma, beta).double() - ref).abs()
    assert (err <= R.ln_bound(ref, slack)).all()
    assert (err <= R.ln_bound_declared(ref, declared)).all()
    if dist == "const-row":
        r = R.ln_const_row(rows)
        assert (x[r] == R.LN_CONST).all()
        assert torch.equal(R.ln_emulate(x, gamma, beta)[r], beta.half())


def test_layer_norm_derived_bound_sees_the_one_pass_variance():
    """sumsq/n - mean^2 in f32 on an offset row: outside the derived bound
    (the measured LN_K cannot see it, torch's own f32 path does the same)."""
    c, rows, dist = 320, 5, "mean64"
    x, gamma, beta = R.ln_inputs(c, rows, dist)
    ref, _, declared = R.ln_reference(c, rows, dist)
    xf = x.float()
    mean = xf.sum(-1, keepdim=True) / c
    var = (xf * xf).sum(-1, keepdim=True) / c - mean * mean
    y = ((xf - mean) * torch.rsqrt(var + R.LN_EPS) * gamma + beta).half()
    assert ((y.double() - ref).abs() > R.ln_bound_declared(ref, declared)).any()


def test_ops_layer_norm_cpu_path_any_width():
    x = torch.randn(3, 77, generator=torch.Generator().manual_seed(1)).half()
    g, b = torch.ones(77), torch.zeros(77)
    ref = F.layer_norm(x.double(), (77,), g.double(), b.double())
    assert (ops.layer_norm(x, g, b).double() - ref).abs().max() < 2e-3


# ---------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------

def test_geglu_constant_is_the_measured_one():
    ratios = {s: R.geglu_f32_ratio(R.geglu_inputs(*s)) for s in R.GEGLU_SHAPES}
    worst = max(ratios, key=ratios.get)
    print(f"torch f32 geglu max ratio {ratios[worst]:.3f} at {worst}")
    assert ratios[worst] == pytest.approx(R.GEGLU_F32_MAX, abs=5e-3)
    assert R.GEGLU_K == pytest.approx(2 * R.GEGLU_F32_MAX, abs=1e-2)


def test_elementwise_inputs_hold_the_explicit_values():
    for n in R.EW_NUMELS[:2]:
        x = R.ew_input(n, 1)
        assert x.numel() == n and x.dtype == torch.float16
        assert x[:8].tolist() == torch.tensor(R.EW_EXPLICIT).half().tolist()
        assert math.copysign(1.0, x[1].item()) == -1.0
    assert R.EW_NUMELS[2] // 8 > R.EW_SWEEP >= 65537
    x = R.geglu_inputs(3, 24)
    assert x.shape == (3, 48)


@pytest.mark.parametrize("rows,inner", R.GEGLU_SHAPES)
def test_cpu_paths_meet_the_elementwise_bounds(rows, inner):
    """The f32 torch paths of ops.* are within the bounds the kernels get."""
    x = R.geglu_inputs(rows, inner)
    ref, ab = R.geglu_ref64(x)
    assert R.within_ulp(ops.geglu(x), ref, ab * R.GEGLU_K * 2.0 ** -23).all()
    a = R.ew_input(rows * inner, 11)
    assert R.within_ulp(ops.silu(a), R.silu_ref64(a)).all()
    b = R.ew_input(rows * inner, 12, shift=2)
    for act in (ops.ACT_NONE, ops.ACT_SILU, ops.ACT_RELU):
        assert R.within_ulp(ops.add_act(a, b, act), R.add_act_ref64(a, b, act)).all()


@pytest.mark.parametrize("shape", R.U8_SHAPES)
def test_u8_fixtures(shape):
    u8 = R.u8_frame(shape)
    n = math.prod(shape)
    assert u8.shape == shape and u8.dtype == torch.uint8
    assert u8.unique().numel() == min(n, 256)
    assert u8.min().item() == 0 and u8.max().item() == 255
    ramp = R.post_ramp(shape)
    assert ramp.shape == shape and ramp.dtype == torch.float16
    assert ramp.min().item() == -1.5 and ramp.max().item() == 1.5
    assert (ramp == 0).any()
    # x = 0 is the one exact tie, and it rounds to even
    assert R.postprocess_ref(h(0.0)).item() == 128
    assert R.postprocess_f32_tie(h(0.0, 2.0 ** -24, 0.5)).tolist() == [True, True, False]
    # the CPU paths of the wrappers meet what the kernels are held to
    assert R.within_ulp(ops.preprocess_from_u8(u8, torch.float16),
                        R.preprocess_ref64(u8)).all()
    got = ops.postprocess_to_u8(ramp)
    diff = got != R.postprocess_ref(ramp)
    assert (R.postprocess_f32_tie(ramp) | ~diff).all()
