"""Per-slot LoRA on the GPU: the lora_delta_ kernel (fragment layout with
exact integers, random data against float64 under a derived bound, argument
checks, graph replay over rewritten tables) and the engine under hip graphs.

References and bounds live in _lora_ref.py. Each test prints its figure
before it asserts.
"""
import pytest
import torch

import _lora_ref as LR
from ai_rtc_agent_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def tables(adapters, scales):
    return (torch.tensor(adapters, dtype=torch.int32, device=DEV),
            torch.tensor(scales, dtype=torch.float32, device=DEV))


# ---------------------------------------------------------------------------
# kernel: fragment layout, exact integers
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("R", [16, 32, 64])
@pytest.mark.parametrize("K", [32, 96])
def test_layout_exact_integers(K, R):
    """Every value is a small integer, so f16 is exact and anything but
    bit-equality is a transposed or permuted fragment. The k order of the
    second product is permuted inside the kernel (the first product's
    accumulators are its operand); B's fragment must follow it."""
    ra, rs = tables([-1, 0, 2, 0], [2.0, 1.0, 2.0, 2.0])
    checked = 0
    for L in (1, 15, 17, 64, 77):
        for N in (16, 48):
            for Ny, col in ((N, 0), (N + 32, 0), (N + 32, 16)):
                x, y, A, B = LR.int_case(4, L, K, N, Ny, R, device=DEV)
                ref, mags = LR.lora_delta_f64(y, x, A, B, ra, rs, col)
                # the precondition of exactness, on the float64 values
                assert mags["t"].abs().max() < 2048 and ref.abs().max() < 2048
                assert mags["d"].abs().max() > 0
                y0 = y.clone()
                out = ops.lora_delta_(y, x, A, B, ra, rs, col)
                assert out is y
                got = y.double().cpu()
                bad = (got != ref).sum().item()
                assert bad == 0, (
                    f"L={L} K={K} N={N} Ny={Ny} col={col} R={R}: {bad} of "
                    f"{ref.numel()} values differ")
                # bare row and the columns outside the range: untouched bits
                assert torch.equal(y[0], y0[0])
                assert torch.equal(y[:, :, :col], y0[:, :, :col])
                assert torch.equal(y[:, :, col + N:], y0[:, :, col + N:])
                checked += 1
    print(f"K={K} R={R}: {checked} shapes bit-equal")


# ---------------------------------------------------------------------------
# kernel: random data against float64
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("R", [32, 16, 64])
def test_random_vs_f64(R):
    """K = N = 320, L = 77 (R = 32 is the issue's case; 16 and 64 take the
    kernel's other two instantiations). The bound is lora_delta_bound: final
    rounding + the intermediate's f16 rounding + f32 accumulation terms,
    all magnitudes from float64."""
    K = N = 320
    L, Bt, n = 77, 4, 3
    g = torch.Generator().manual_seed(R)
    x = torch.randn(Bt, L, K, generator=g).half().to(DEV)
    y = torch.randn(Bt, L, N + 64, generator=g).half().to(DEV)
    A = (torch.randn(n, R, K, generator=g) * 0.05).half().to(DEV)
    B = (torch.randn(n, N, R, generator=g) * 0.05).half().to(DEV)
    ra, rs = tables([2, -1, 0, 1], [1.0, 3.0, -0.75, 0.0])
    col = 32
    ref, mags = LR.lora_delta_f64(y, x, A, B, ra, rs, col)
    # precondition: the intermediate sits far inside f16's normal range
    tmax = mags["abs_t"].max().item()
    tmed = mags["t"].abs()[mags["t"] != 0].median().item()
    assert tmax < 65504 / 64 and tmed > 2.0 ** -14 * 64, (tmax, tmed)
    bound = LR.lora_delta_bound(ref, mags, rs, K, R, N, col)
    y0 = y.clone()
    ops.lora_delta_(y, x, A, B, ra, rs, col)
    err = (y.double().cpu() - ref).abs()
    inside = bound > 0
    ratio = (err[inside] / bound[inside]).max().item()
    print(f"R={R}: max err {err.max().item():.3e}, max err/bound {ratio:.3f}, "
          f"max |t| sum {tmax:.2f}")
    assert ratio <= 1.0
    assert torch.equal(y[1], y0[1])
    assert torch.equal(y[:, :, :col], y0[:, :, :col])
    assert torch.equal(y[:, :, col + N:], y0[:, :, col + N:])
    # scale 0 on an assigned row: y + 0 rounds to y
    assert torch.equal(y[3], y0[3])
    assert (err[~inside] == 0).all()


# ---------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------

def _good(K=32, N=16, Ny=16, R=16, L=3, Bt=2, n=2):
    h = dict(dtype=torch.float16, device=DEV)
    return dict(
        y=torch.zeros(Bt, L, Ny, **h), x=torch.ones(Bt, L, K, **h),
        A=torch.ones(n, R, K, **h), B=torch.ones(n, N, R, **h),
        row_adapter=torch.zeros(Bt, dtype=torch.int32, device=DEV),
        row_scale=torch.ones(Bt, dtype=torch.float32, device=DEV),
        col_offset=0)


def _ext_call(a):
    return ops.hip_ext().lora_delta_(a["y"], a["x"], a["A"], a["B"],
                                     a["row_adapter"], a["row_scale"],
                                     a["col_offset"])


BAD = {
    "K % 32": lambda: _good(K=48),
    "N % 16": lambda: _good(N=24, Ny=32),
    "col_offset % 16": lambda: {**_good(Ny=32), "col_offset": 8},
    "col_offset + N > Ny": lambda: {**_good(Ny=16), "col_offset": 16},
    "R = 8": lambda: _good(R=8),
    "R = 48": lambda: _good(R=48),
    "Ny % 4": lambda: _good(Ny=18),
    "x f32": lambda: {**_good(), "x": _good()["x"].float()},
    "y f32": lambda: {**_good(), "y": _good()["y"].float()},
    "A f32": lambda: {**_good(), "A": _good()["A"].float()},
    "B bf16": lambda: {**_good(), "B": _good()["B"].bfloat16()},
    "row_adapter i64": lambda: {**_good(), "row_adapter": _good()["row_adapter"].long()},
    "row_scale f16": lambda: {**_good(), "row_scale": _good()["row_scale"].half()},
    "row_adapter count": lambda: {**_good(), "row_adapter": torch.zeros(
        3, dtype=torch.int32, device=DEV)},
    "x not contiguous": lambda: {**_good(), "x": torch.ones(
        2, 3, 64, dtype=torch.float16, device=DEV)[:, :, ::2]},
    "y not contiguous": lambda: {**_good(), "y": torch.zeros(
        2, 3, 32, dtype=torch.float16, device=DEV)[:, :, :16]},
    "A on the host": lambda: {**_good(), "A": _good()["A"].cpu()},
    "row_scale on the host": lambda: {**_good(), "row_scale": _good()["row_scale"].cpu()},
    "A's K": lambda: {**_good(), "A": torch.ones(
        2, 16, 64, dtype=torch.float16, device=DEV)},
    "B's R": lambda: {**_good(), "B": torch.ones(
        2, 16, 32, dtype=torch.float16, device=DEV)},
    "y's tokens": lambda: {**_good(), "y": torch.zeros(
        2, 4, 16, dtype=torch.float16, device=DEV)},
    "x misaligned": lambda: {**_good(), "x": torch.ones(
        2 * 3 * 32 + 1, dtype=torch.float16, device=DEV)[1:].view(2, 3, 32)},
}


@pytest.mark.parametrize("what", list(BAD))
def test_refused_arguments(what):
    a = BAD[what]()
    y0 = a["y"].clone()
    with pytest.raises(RuntimeError, match="lora_delta_|must be"):
        _ext_call(a)
    torch.cuda.synchronize()
    assert torch.equal(a["y"], y0), "a refused call must launch nothing"


def test_index_limit_is_refused():
    """Element counts past 31 bits are refused. The check needs a real
    tensor: the smallest over-limit operand is B = (1, 2^26, 32) f16, 4 GiB,
    allocated and never touched."""
    h = dict(dtype=torch.float16, device=DEV)
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:  # before any work: a small or busy card cannot show it
        pytest.skip("needs 8 GiB of free device memory")
    a = _good(Bt=1, L=1)
    a["A"] = torch.ones(1, 32, 32, **h)
    a["B"] = torch.empty(1, 1 << 26, 32, **h)
    a["y"] = torch.empty(1, 1, 1 << 26, **h)
    with pytest.raises(RuntimeError, match="2\\^31"):
        _ext_call(a)


def test_interface_checks_before_dispatch():
    a = _good()
    with pytest.raises(ValueError):
        ops.lora_delta_(a["y"], a["x"], a["A"], a["B"],
                        a["row_adapter"].long(), a["row_scale"])
    with pytest.raises(ValueError):
        ops.lora_delta_(a["y"], a["x"], a["A"], a["B"], a["row_adapter"],
                        a["row_scale"], col_offset=16)


# ---------------------------------------------------------------------------
# graph replay over rewritten tables and bank
# ---------------------------------------------------------------------------

def test_graph_follows_tables_and_bank():
    L, K, N, R = 17, 96, 48, 32
    x, y_init, A, B = LR.int_case(4, L, K, N, N + 32, R, device=DEV)
    ra, rs = tables([-1, 0, 2, 0], [1.0, 1.0, 2.0, 2.0])
    y = y_init.clone()
    ops.lora_delta_(y, x, A, B, ra, rs, 16)  # warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    y.copy_(y_init)
    with torch.cuda.graph(g):
        ops.lora_delta_(y, x, A, B, ra, rs, 16)
    y.copy_(y_init)
    g.replay()
    first = y.clone()
    # rewrite the tables and bank index 1 in place
    ra.copy_(torch.tensor([1, -1, 0, 2], dtype=torch.int32))
    rs.copy_(torch.tensor([2.0, 1.0, 1.0, 1.0]))
    A[1].copy_(A[2].flip(0))
    B[1].copy_(B[0].flip(1))
    y.copy_(y_init)
    g.replay()
    torch.cuda.synchronize()
    eager = y_init.clone()
    ops.lora_delta_(eager, x, A, B, ra, rs, 16)
    assert torch.equal(y, eager)
    assert not torch.equal(y, first)
    assert torch.equal(y[1], y_init[1]) and not torch.equal(y[0], y_init[0])


# ---------------------------------------------------------------------------
# engine: tiny family, hip graphs, fbs = 2
# ---------------------------------------------------------------------------

from ai_rtc_agent_amd.config import EngineConfig  # noqa: E402
from ai_rtc_agent_amd.engine import StreamDiffusionEngine  # noqa: E402
from ai_rtc_agent_amd.models.lora import fuse_lora_state_dict  # noqa: E402

FBS, N_FRAMES = 2, 4


def make_engine(overlap=True, lora_adapters=0, **kw):
    args = dict(model_family="tiny", width=64, height=64, device="cuda",
                acceleration="hip", use_hip_graph=True,
                pipeline_overlap=overlap, use_lcm_lora=False,
                t_index_list=[10, 30], cfg_type="self", guidance_scale=1.5,
                frame_buffer_size=FBS, lora_adapters=lora_adapters,
                lora_max_rank=8)
    args.update(kw)
    eng = StreamDiffusionEngine(EngineConfig(**args))
    eng.prepare()
    return eng


def frames():
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, 256, (N_FRAMES, FBS, 64, 64, 3), generator=g,
                         dtype=torch.uint8).to(DEV)


def run(eng, lo=0, hi=N_FRAMES):
    outs = []
    for i in range(lo, hi):
        out = eng(frames()[i])
        eng.sync_output()
        outs.append(out.clone())
    return torch.stack(outs)


def graph_objects(eng):
    if eng._pipelined:
        assert eng._graph is True
        return list(eng._g1) + list(eng._g2)
    assert eng._graph is not None
    return [eng._graph]


def adapter_for(eng, **kw):
    return LR.attention_lora(eng.unet, rank=4, seed=21, std=0.3, **kw)


@pytest.mark.parametrize("overlap", [True, False])
def test_engine_slots_under_graphs(overlap):
    """Adapters are assigned, switched and loaded AFTER the first frame, when
    the graphs exist: every change shows on the next frame, the graph objects
    stay the same, and slot 1 (no adapter) stays bit-equal to an engine
    without the feature."""
    base = run(make_engine(overlap))
    eng = make_engine(overlap, lora_adapters=2)
    X = adapter_for(eng)
    Kq = adapter_for(eng, only="attn2.to_k")
    eng.load_adapter(0, X, name="x")
    out0 = run(eng, 0, 1)
    assert torch.equal(out0, base[:1]), "capacity on, nothing assigned"
    graphs = graph_objects(eng)

    eng.update_lora(adapter="x", slot=0)
    out1 = run(eng, 1, 2)
    assert torch.equal(out1[:, 1], base[1:2, 1])
    assert not torch.equal(out1[:, 0], base[1:2, 0])

    # the same index reloaded with an adapter on attn2.to_k alone: the
    # slot's static K|V rows must follow
    eng.load_adapter(0, Kq, name="k")
    out2 = run(eng, 2, 3)
    assert torch.equal(out2[:, 1], base[2:3, 1])
    assert not torch.equal(out2[:, 0], base[2:3, 0])

    eng.update_lora(adapter=None, slot=0)
    run(eng, 3, 4)
    now = graph_objects(eng)
    assert len(now) == len(graphs) and all(a is b for a, b in zip(now, graphs))

    # the three steps against engines that were in that state from frame 0
    ref = make_engine(overlap, lora_adapters=2)
    ref.load_adapter(0, X, name="x")
    run(ref, 0, 1)
    ref.update_lora(adapter="x", slot=0)
    assert torch.equal(run(ref, 1, 2), out1)


def test_attn2_to_k_alone_under_graphs():
    base = run(make_engine())
    eng = make_engine(lora_adapters=1)
    eng.load_adapter(0, adapter_for(eng, only="attn2.to_k"))
    run(eng, 0, 1)
    eng.update_lora(adapter=0, slot=0)
    out = run(eng, 1, N_FRAMES)
    assert torch.equal(out[:, 1], base[1:, 1])
    assert not torch.equal(out[:, 0], base[1:, 0])


def level_stats(a, b):
    d = (a - b).abs().float()
    return d.mean().item(), d.flatten().quantile(0.99).item(), d.max().item()


@pytest.mark.parametrize("cfg_type,t_index_list",
                         [("self", [10, 30]), ("none", [30])])
def test_unfused_f16_against_the_f16_noise_floor(cfg_type, t_index_list):
    """Slot 0 with adapter X unfused, in f16 under graphs, against a float32
    eager engine with X fused; the yardstick is an f16 engine with X fused,
    the f16 noise floor of the same network.

    Both f16 engines run the same kernels on every op except the targeted
    projections. There the fused engine rounds the projection's output to
    f16 once. The unfused one rounds that output, the rank-R intermediate
    (which scales only the delta part), and the sum with the delta: three
    f16 roundings where the fused engine has one, each at most u16 of a
    value no larger than the output. To first order the errors add, so the
    unfused error is at most 3x the floor even if every bit of the floor
    came from the targeted projections; half a u8 level is added because
    both errors are measured on quantized frames.

    The statistic is the MEAN |levels| over slot 0's frames. The maximum is
    useless here: the random-weight tiny UNet saturates single pixels under
    f16 rounding (both routes read 241 levels at their worst pixel).

    Two configurations: the two-step "self" stream, and one step with
    cfg_type "none", the fewest UNet passes between input and picture, where
    f16 rounding is amplified least.

    Measured on one MI355X for ("self", [10, 30]), mean / 99th percentile /
    max |levels| against the float32 engine with X fused:
      unfused f16            10.511 / 117 / 241
      fused f16 (the floor)  10.474 / 117 / 241
      f16 WITHOUT the adapter (a wrong picture)  31.686 / 156 / 255
    The floor of this network is high, so 3 * floor + 0.5 = 31.92 lies 0.24
    levels above the wrong picture's 31.69: the derived bound alone would
    not reject it. Two further requirements are therefore asserted, as
    sanity checks and not as bounds: the unfused picture is nearer to the
    reference than the picture without the adapter, and the adapter moves
    the picture by more than the floor (otherwise the comparison says
    nothing). The kernel itself is bounded by the float64 op test above.
    """
    X = None
    outs = {}
    for key, kw in (("f32", dict(device="cuda", dtype="float32",
                                 acceleration="eager", use_hip_graph=False)),
                    ("f16_fused", {}), ("f16_unfused", dict(lora_adapters=1)),
                    ("f16_bare", {})):
        eng = make_engine(cfg_type=cfg_type, t_index_list=t_index_list, **kw)
        if X is None:
            X = adapter_for(eng)
        if key == "f16_unfused":
            eng.load_adapter(0, X)
            eng.update_lora(adapter=0, slot=0)
        elif key != "f16_bare":
            fuse_lora_state_dict(eng.unet, X)
            eng.refresh_weights()
        outs[key] = run(eng)[:, 0].int()
    unfused = level_stats(outs["f16_unfused"], outs["f32"])
    floor = level_stats(outs["f16_fused"], outs["f32"])
    wrong = level_stats(outs["f16_bare"], outs["f32"])
    for name, st in (("unfused f16", unfused), ("fused f16 (floor)", floor),
                     ("no adapter f16 (a wrong picture)", wrong)):
        print(f"{name} vs fused f32: mean {st[0]:.3f}, p99 {st[1]:.0f}, "
              f"max {st[2]:.0f} levels")
    bound = 3 * floor[0] + 0.5
    print(f"bound {bound:.3f}: rejects the picture without the adapter: "
          f"{wrong[0] > bound}")
    assert unfused[0] <= bound
    assert wrong[0] > 2 * floor[0], "the adapter does not move the picture enough"
    assert unfused[0] < 0.5 * wrong[0]


def test_index_past_the_bank_is_a_bare_row():
    x, y, A, B = LR.int_case(4, 17, 32, 16, 16, 16, n_adapters=2, device=DEV)
    ra, rs = tables([2, 1, 7, 0], [1.0, 1.0, 1.0, 1.0])  # 2 and 7: past the bank
    ref, _ = LR.lora_delta_f64(y, x, A, B, ra, rs)
    y0 = y.clone()
    ops.lora_delta_(y, x, A, B, ra, rs)
    assert torch.equal(y[0], y0[0]) and torch.equal(y[2], y0[2])
    assert torch.equal(y.double().cpu(), ref)
