"""Per-session controls on the GPU: the airtc_rcfg_apply kernel against the
aten chain it replaces, and the engine triangle under pipelined hipGraphs.

Rounding: the kernel rounds to f16 after each arithmetic step (f32 math:
the f32 result is rounded to f32, then to f16). Three references:

- the CPU aten chain, bound 1 f16 ulp on every shape (measured: 0);
- the chain with its rounding written out on the device (`stepwise`: f32
  tensor ops, `.half()` after each), exact on every shape;
- the aten f16 chain on the device, exact wherever aten runs its vectorized
  elementwise kernel, i.e. when the element count is a whole number of its
  blocks (AT_FULL below) — which is every latent size the engine serves.

The third is not asserted on the other shapes, for a reason in aten's own op
semantics: measured on the MI355X (torch 2.10 / ROCm 7.0), the kernel that
aten runs for a partial block multiplies an f16 tensor by a Python scalar
with ONE rounding (f32 scalar x f16 straight to f16), its vectorized kernel
with two (to f32, then to f16), like its CPU kernel and like ours. The two
aten kernels disagree with each other on products that the f32 rounding
moves onto an f16 tie (3 of 384 elements for delta = 0.7; e.g. 0.7f *
1.4501953125 = 1.0146484375 in one, 1.015625 in the other), and the
subtraction that follows can cancel, so the final outputs then differ by many
ulp (32 seen) although one intermediate differs by one.
"""
import pytest
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import EngineConfig
from ai_rtc_agent_amd.engine import StreamDiffusionEngine
from ai_rtc_agent_amd.engine.rcfg import ResidualCFG

pytestmark = pytest.mark.gpu

B, FBS = 6, 2
MODES = ("self", "initialize", "full")
# per_b = 64, 24 (8 * odd), 12 (no multiple of 8: the scalar path); then a
# 512x512 latent batch (many blocks) and two sizes past the capped grid
# (2048 blocks x 256 threads), one per path, so the grid-stride loop runs
SHAPES = ((B, 4, 4, 4), (B, 1, 6, 4), (B, 1, 3, 4),
          (B, 64, 64, 4), (B, 512, 96, 16), (B, 301, 301, 1))
G_ROWS = (1.5, 3.0, 0.5, 2.25, 1.0, 7.5)
D_ROWS = (1.0, 0.5, 0.7, 1.0, 0.9, 0.3)


def rcfg_inputs(mode, shape, seed=0):
    gen = torch.Generator().manual_seed(seed)
    rows = {"self": B, "initialize": B + FBS, "full": 2 * B}[mode]
    eps = torch.randn((rows, *shape[1:]), generator=gen).half()
    stock = torch.randn(shape, generator=gen).half()
    return eps, stock


def scalar_chain(mode, eps, stock, g, delta):
    """ResidualCFG's scalar path (the aten chain) on clones, on the device
    the inputs live on. Returns (out, stock after)."""
    r = ResidualCFG(mode, g, delta, runtime=g <= 1.0)
    r.stock_noise = stock.clone()
    out = r.apply(eps.clone(), FBS)
    return out, r.stock_noise


def kernel_rows(mode, eps, stock, g_rows, d_rows):
    g_eff = [max(g, 1.0) for g in g_rows]
    f32 = dict(dtype=torch.float32, device="cuda")
    stock = stock.clone()
    if mode == "full":
        out = ops.rcfg_apply("full", eps.clone(), FBS, g=torch.tensor(g_eff, **f32))
        return out, stock
    gm1 = torch.tensor([g - 1.0 for g in g_eff], dtype=torch.float64).float().cuda()
    out = ops.rcfg_apply(mode, eps.clone(), FBS, stock=stock, gm1=gm1,
                         delta=torch.tensor(d_rows, **f32))
    return out, stock


AT_FULL = 4096  # elements: a multiple of every aten elementwise block size


def stepwise(mode, eps, stock, g_rows, d_rows):
    """The chain with per-row f32 coefficients and each rounding explicit:
    f32 tensor ops, .half() after every step. Returns out."""
    sh = (-1, *([1] * (eps.dim() - 1)))
    dev = eps.device
    g_eff = [max(g, 1.0) for g in g_rows]
    if mode == "full":
        g = torch.tensor(g_eff, dtype=torch.float32, device=dev).view(sh)
        u, c = eps[:B].float(), eps[B:].float()
        df = (c - u).half().float()
        return (u + (g * df).half().float()).half()
    gm1 = torch.tensor([g - 1.0 for g in g_eff], dtype=torch.float64).float().to(dev).view(sh)
    dl = torch.tensor(d_rows, dtype=torch.float32, device=dev).view(sh)
    e = eps[eps.shape[0] - B:].float()
    s = stock.clone()
    if mode == "initialize":
        s[:FBS] = eps[:FBS]
    df = (e - (dl * s.float()).half().float()).half().float()
    return (e + (gm1 * df).half().float()).half()


def ulp_distance(a, b):
    """f16 tensors -> distance in units in the last place (monotone integer
    image of the f16 line)."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs().max().item()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_kernel_uniform_equals_aten_chain(mode, shape):
    eps, stock = rcfg_inputs(mode, shape)
    want, want_stock = scalar_chain(mode, eps.cuda(), stock.cuda(), 1.5, 0.7)
    got, got_stock = kernel_rows(mode, eps.cuda(), stock.cuda(), [1.5] * B, [0.7] * B)
    cpu, cpu_stock = scalar_chain(mode, eps, stock, 1.5, 0.7)
    torch.cuda.synchronize()
    assert got.shape == shape and got.dtype == torch.float16
    print("ulp vs device chain", ulp_distance(got, want),
          "vs cpu chain", ulp_distance(got.cpu(), cpu))
    assert ulp_distance(got.cpu(), cpu) <= 1
    assert torch.equal(got, stepwise(mode, eps.cuda(), stock.cuda(), [1.5] * B, [0.7] * B))
    if got.numel() % AT_FULL == 0:  # aten's vectorized kernel: module docstring
        assert torch.equal(got, want)
    if mode != "full":
        assert torch.equal(got_stock, want_stock)
        assert torch.equal(got_stock.cpu(), cpu_stock)  # the shift is a copy


@pytest.mark.parametrize("shape", SHAPES[:4])
@pytest.mark.parametrize("mode", MODES)
def test_kernel_per_row_equals_chain_per_row(mode, shape):
    eps, stock = rcfg_inputs(mode, shape, seed=1)
    eps_d, stock_d = eps.cuda(), stock.cuda()
    got, got_stock = kernel_rows(mode, eps_d, stock_d, G_ROWS, D_ROWS)
    eps_c = eps_d[eps_d.shape[0] - B:]
    assert torch.equal(got, stepwise(mode, eps_d, stock_d, G_ROWS, D_ROWS))
    for r in range(B):
        want, want_stock = scalar_chain(mode, eps_d, stock_d, G_ROWS[r], D_ROWS[r])
        cpu, _ = scalar_chain(mode, eps, stock, G_ROWS[r], D_ROWS[r])
        assert ulp_distance(got[r].cpu(), cpu[r]) <= 1, f"row {r}"
        if got.numel() % AT_FULL == 0:  # aten's vectorized kernel
            assert torch.equal(got[r], want[r]), f"row {r}"
        if mode != "full":
            assert torch.equal(got_stock, want_stock)
            if G_ROWS[r] <= 1.0:
                assert torch.equal(got[r], eps_c[r]), f"row {r}"


@pytest.mark.parametrize("shape", SHAPES[:4])
def test_kernel_product_within_one_ulp_of_device_aten(shape):
    """The one step where rounding models can differ, delta * stock, read
    out of the kernel itself: with eps = 0 and gm1 = -1 the self step is
    0 + (-1)*(0 - delta*stock) = the kernel's own rounded product (negation
    is exact). Against aten's `delta * stock` on the device, whichever of
    its kernels runs: at most 1 f16 ulp, uniform and per row."""
    _, stock = rcfg_inputs("self", shape, seed=2)
    stock = stock.cuda()
    eps = torch.zeros_like(stock)
    m1 = torch.full((B,), -1.0, dtype=torch.float32, device="cuda")
    sh = (-1, *([1] * (stock.dim() - 1)))
    for d_rows in ([0.7] * B, list(D_ROWS)):
        dl = torch.tensor(d_rows, dtype=torch.float32, device="cuda")
        got = ops.rcfg_apply("self", eps, FBS, gm1=m1, delta=dl, stock=stock.clone())
        want = torch.cat([d_rows[r] * stock[r:r + 1] for r in range(B)])
        assert ulp_distance(got, want) <= 1
        # and it is the product rounded to f32, then to f16
        assert torch.equal(got, (dl.view(sh) * stock.float()).half())


def test_kernel_rejects_aliasing_and_bad_shapes():
    eps, stock = rcfg_inputs("self", SHAPES[0])
    eps, stock = eps.cuda(), stock.cuda()
    one = torch.ones(B, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="alias"):
        ops.rcfg_apply("self", eps, FBS, gm1=one, delta=one, stock=eps)
    with pytest.raises(RuntimeError):
        ops.rcfg_apply("self", eps, FBS, gm1=one[:4], delta=one[:4], stock=stock)
    with pytest.raises(RuntimeError):
        ops.rcfg_apply("self", eps, 4, gm1=one, delta=one, stock=stock)  # 6 % 4
    with pytest.raises(RuntimeError):
        ops.rcfg_apply("full", eps, FBS, g=one)  # needs 2B rows
    with pytest.raises(RuntimeError):
        ops.rcfg_apply("self", eps, FBS, gm1=one, delta=one, stock=stock[:, :2])


# ---------------------------------------------------------------------------
# engine: acceleration hip, hipGraph on, pipelined graphs
# ---------------------------------------------------------------------------
PROMPT_A = "a watercolour painting of a harbour at dawn"
PROMPT_B = "neon cyberpunk alley in heavy rain"
N_FRAMES = 5


def make_engine(**kw):
    args = dict(model_family="tiny", width=64, height=64, device="cuda",
                acceleration="hip", use_hip_graph=True, pipeline_overlap=True,
                use_lcm_lora=False, t_index_list=[10, 30], cfg_type="self",
                guidance_scale=1.5, frame_buffer_size=FBS)
    args.update(kw)
    eng = StreamDiffusionEngine(EngineConfig(**args))
    eng.prepare()
    return eng


def frames():
    gen = torch.Generator().manual_seed(7)
    return torch.randint(0, 256, (N_FRAMES, FBS, 64, 64, 3), generator=gen,
                         dtype=torch.uint8).cuda()


def run_clone(eng, frame):
    out = eng(frame)
    eng.sync_output()
    return out.clone()


def triangle(setup, a, b, host_frames=False, **kw):
    """Per-slot controls (a, b), (a, a), (b, b), set AFTER the first frame
    (the graphs are captured by then); outputs of the frames that follow.
    Also asserts that no update dropped or re-captured a graph.
    host_frames: the frames come from the CPU, so every call allocates its
    upload on the caller's stream right after the updates, while stream A
    may not have run the updates' copies yet."""
    fr = frames().cpu() if host_frames else frames()
    outs = []
    for s0, s1 in ((a, b), (a, a), (b, b)):
        eng = make_engine(**kw)
        run_clone(eng, fr[0])
        assert eng._pipelined and eng._graph is True
        g1, g2 = list(eng._g1), list(eng._g2)
        setup(eng, s0, 0)
        setup(eng, s1, 1)
        outs.append(torch.stack([run_clone(eng, f) for f in fr[1:]]))
        assert all(x is y for x, y in zip(eng._g1, g1)), "g1 re-captured"
        assert all(x is y for x, y in zip(eng._g2, g2)), "g2 re-captured"
        assert len(eng._g1) == len(g1) == 2 and eng._graph is True
    return outs


def assert_triangle(x, y, z):
    assert not torch.equal(y[:, 0], z[:, 0]), "the control changes nothing"
    assert not torch.equal(y[:, 1], z[:, 1]), "the control changes nothing"
    assert torch.equal(x[:, 0], y[:, 0])
    assert torch.equal(x[:, 1], z[:, 1])


def test_engine_per_slot_prompt_under_graphs():
    x, y, z = triangle(lambda e, v, s: e.update_prompt(v, slot=s),
                       PROMPT_A, PROMPT_B)
    assert_triangle(x, y, z)


def test_engine_per_slot_guidance_under_graphs():
    x, y, z = triangle(lambda e, v, s: e.update_guidance(v, slot=s), 1.0, 2.0)
    assert_triangle(x, y, z)


def test_engine_per_slot_t_index_with_host_frames_under_graphs():
    """The coefficient tensors of a t_index_list update are built on the
    caller's stream and copied on stream A. Host frames make the caller's
    stream allocate (the upload) straight after the update: the freed
    coefficient blocks must not be handed out before stream A has read
    them."""
    def setup(e, v, s):
        e.update_t_index_list(v, slot=s)
        # small allocations on the caller's stream, the pool the freed
        # coefficient tensors went back to
        junk = [torch.full((64,), float("nan"), device="cuda", dtype=torch.float32)
                for _ in range(32)]
        del junk

    x, y, z = triangle(setup, [10, 30], [5, 45], host_frames=True)
    assert_triangle(x, y, z)
    # and the replica-wide path
    fr = frames().cpu()
    a, b = make_engine(), make_engine(t_index_list=[5, 45])
    run_clone(a, fr[0])
    a.update_t_index_list([5, 45])
    _ = [torch.full((64,), float("nan"), device="cuda") for _ in range(32)]
    run_clone(b, fr[0])
    for f in fr[1:3]:
        run_clone(a, f), run_clone(b, f)  # stage buffers turn over
    for f in fr[3:]:
        assert torch.equal(run_clone(a, f), run_clone(b, f))


def test_engine_per_slot_t_index_and_reset_under_graphs():
    """t_index_list per slot, then reset_slot: the slot goes back to the
    defaults without a re-capture and the other slot never notices."""
    fr = frames()
    eng, ref = make_engine(), make_engine()
    run_clone(eng, fr[0])
    run_clone(ref, fr[0])
    g1 = list(eng._g1)
    eng.update_t_index_list([5, 45], slot=1)
    a, b = run_clone(eng, fr[1]), run_clone(ref, fr[1])
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    eng.reset_slot(1)
    assert eng.slot_controls(1) == ref.slot_controls(1)
    outs = torch.stack([run_clone(eng, f) for f in fr[2:]])
    # fresh = the post-prepare() state: an eager engine (capturing first
    # advances the stream-batch state by its warm-up steps; replay itself
    # equals eager, test_engine_gpu.py::test_graph_replay_matches_eager)
    fresh = make_engine(use_hip_graph=False)
    want = torch.stack([run_clone(fresh, f) for f in fr[2:]])
    assert torch.equal(outs[:, 1], want[:, 1])
    assert all(x is y for x, y in zip(eng._g1, g1))


@pytest.mark.parametrize("cfg_type", MODES)
def test_engine_kernel_step_equals_aten_chain_step(cfg_type):
    """Swapping the kernel in changes nothing: the engine with the fused
    kernel equals the same engine taking ResidualCFG's scalar aten chain
    (its per-row tensors dropped), both captured. 128x128 frames: the
    4 x 16 x 16 x 4 latent batch is AT_FULL elements, so aten runs the
    kernel it runs at every served size (module docstring)."""
    gen = torch.Generator().manual_seed(11)
    fr = torch.randint(0, 256, (3, FBS, 128, 128, 3), generator=gen,
                       dtype=torch.uint8).cuda()
    eng = make_engine(cfg_type=cfg_type, guidance_scale=1.3, delta=0.7,
                      width=128, height=128)
    chain = make_engine(cfg_type=cfg_type, guidance_scale=1.3, delta=0.7,
                        width=128, height=128)
    assert eng.rcfg.gm1_rows is not None and eng.rcfg.gm1_rows.is_cuda
    assert eng.rcfg.stock_noise.numel() % AT_FULL == 0
    chain.rcfg.g_rows = chain.rcfg.gm1_rows = chain.rcfg.delta_rows = None
    assert chain.rcfg.active
    for f in fr:
        assert torch.equal(run_clone(eng, f), run_clone(chain, f))
