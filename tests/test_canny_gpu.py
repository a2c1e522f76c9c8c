"""The Canny hint kernel (ops/csrc/canny.hip) against the torch form of the
operator, bit for bit, and the engine's canny ControlNet path under
pipelined hipGraphs. The operator is integer arithmetic up to the final
store, so every comparison is torch.equal.

The kernel works on 32x32 tiles with a halo of reach + 4; the sizes below
sit under one tile, are no multiple of it and span several tiles on both
axes, and the chain cases run a weak edge across tile boundaries, which is
what a halo one pixel short gets wrong.
"""
import pytest
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import EngineConfig
from ai_rtc_agent_amd.engine import StreamDiffusionEngine
from test_canny_cpu import THR, chain_frame, engine_frames, grey, scene, unzero

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (3, 5), (8, 8), (33, 70), (64, 64), (97, 131), (130, 40))
REACHES = (0, 1, 2, 16, 32)


def reference(frames, thr, reach, dtype=torch.float16):
    """The torch path, on the CPU, for (B,H,W,3) u8 CPU frames."""
    assert not frames.is_cuda
    return ops.canny_hint(frames, thr, reach, dtype)


def kernel(frames, thr, reach, dtype=torch.float16, out=None):
    if isinstance(thr, torch.Tensor):
        thr = thr.cuda()
    res = ops.canny_hint(frames.cuda(), thr, reach, dtype, out=out)
    torch.cuda.synchronize()
    return res


def assert_same(frames, thr, reach, dtype=torch.float16):
    want = reference(frames, thr, reach, dtype)
    got = kernel(frames, thr, reach, dtype)
    assert got.dtype == dtype and got.shape == frames.shape and got.is_contiguous()
    bad = int((got.cpu() != want).sum())
    assert bad == 0, f"{bad} of {want.numel()} values differ"
    return want


_SCENES = {}


def scenes(size):
    """Two scenes of a size (computed once per size)."""
    if size not in _SCENES:
        _SCENES[size] = torch.stack([scene(*size), scene(*size, seed=1)])
    return _SCENES[size]


@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_torch_path(size, reach):
    want = assert_same(scenes(size), THR, reach)
    if min(size) >= 33:
        assert want.any(), "the scene has no edges: nothing was compared"


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_per_row_thresholds(dtype):
    s = torch.stack([scene(97, 131, seed=i) for i in range(3)])
    thr = torch.tensor([(20, 60), (50, 100), (90, 400)], dtype=torch.int32)
    want = assert_same(s, thr, 8, dtype)
    assert len({int(w.sum()) for w in want}) == 3  # the thresholds matter
    # and the tensor is read at run time: the same launch arguments follow
    # an in-place write
    d = thr.cuda()
    x = s.cuda()
    a = ops.canny_hint(x, d, 8, dtype)
    d.copy_(torch.tensor([(90, 400), (20, 60), (50, 100)], dtype=torch.int32))
    b = ops.canny_hint(x, d, 8, dtype)
    assert torch.equal(b.cpu(), reference(s, d.cpu(), 8, dtype)) and not torch.equal(a, b)


@pytest.mark.parametrize("transpose", [False, True], ids=["row", "column"])
@pytest.mark.parametrize("reach", [4, 16, 32])
def test_chain_across_tile_boundaries(reach, transpose):
    # the faint line runs from column 30 to 130 along row 33: it crosses the
    # tile boundaries 32, 64, 96 and 128 and lies one row past boundary 32
    f = chain_frame(48, 140, 33, 30, 100, transpose).unsqueeze(0)
    want = assert_same(f, THR, reach)
    strong = reference(f, THR, 0)
    assert int(want[..., 0].sum() - strong[..., 0].sum()) == reach


@pytest.mark.parametrize("where", ["top", "left", "bottom", "right"])
def test_only_gradient_on_the_border(where):
    """Clamp to the image, not to the window: the one strong gradient of the
    frame lies on its first or last row or column (a 1 px line there), in
    a frame of several tiles so that most windows hang over the border."""
    img = torch.full((70, 100), 40.0)
    if where == "top":
        img[0, 10:90] = 220.0
    elif where == "bottom":
        img[-1, 10:90] = 220.0
    elif where == "left":
        img[5:65, 0] = 220.0
    else:
        img[5:65, -1] = 220.0
    f = grey(img).unsqueeze(0)
    for reach in (0, 16):
        want = assert_same(f, (20, 60), reach)
        assert want.any()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_no_stray_writes(dtype):
    """out= embedded in a larger 0xAB-filled allocation at an odd element
    offset (so its rows start at every alignment), other batch rows
    pre-filled: only the addressed rows change, and only inside out."""
    B, H, W = 2, 33, 70
    s = scenes((H, W))
    n = B * H * W * 3
    esize = torch.empty((), dtype=dtype).element_size()
    for off in (1, 2, 5):  # elements
        pad = 64
        raw = torch.full(((pad + off + n + pad) * esize,), 0xAB, dtype=torch.uint8,
                         device="cuda")
        typed = raw.view(dtype)
        out = typed[pad + off:pad + off + n].view(B, H, W, 3)
        assert out.is_contiguous()
        got = kernel(s, THR, 16, dtype, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out.cpu(), reference(s, THR, 16, dtype))
        head = raw[:(pad + off) * esize]
        tail = raw[(pad + off + n) * esize:]
        assert bool((head == 0xAB).all()) and bool((tail == 0xAB).all())
    # one batch row addressed through a view: the others keep their fill
    full = torch.full((3, H, W, 3), 7.0, dtype=dtype, device="cuda")
    kernel(s[:1], THR, 16, dtype, out=full[1:2])
    assert bool((full[0] == 7.0).all()) and bool((full[2] == 7.0).all())
    assert torch.equal(full[1:2].cpu(), reference(s[:1], THR, 16, dtype))


def test_kernel_captures_into_a_graph():
    s = scenes((97, 131)).cuda()
    thr = torch.tensor([THR, THR], dtype=torch.int32, device="cuda")
    out = torch.empty(s.shape, dtype=torch.float16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.canny_hint(s, thr, 16, torch.float16, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.canny_hint(s, thr, 16, torch.float16, out=out)
    for pair in ((20, 60), (90, 400)):
        thr.copy_(torch.tensor([pair, pair], dtype=torch.int32))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), reference(s.cpu(), pair, 16))


def test_rejects_what_the_kernel_cannot_take():
    s = scenes((8, 8)).cuda()
    with pytest.raises(ValueError):
        ops.canny_hint(s, THR, 33)
    with pytest.raises(ValueError):
        ops.canny_hint(s, torch.tensor([THR, THR], dtype=torch.int32), 4)  # CPU thr
    with pytest.raises(TypeError):
        ops.canny_hint(s, THR, 4, torch.bfloat16)


# ---------------------------------------------------------------------------
# engine: acceleration hip, hipGraph on, pipelined graphs
# ---------------------------------------------------------------------------
FBS = 2


def make_engine(**kw):
    args = dict(model_family="tiny", width=64, height=64, device="cuda",
                acceleration="hip", use_hip_graph=True, pipeline_overlap=True,
                use_lcm_lora=False, t_index_list=[18, 26, 35, 45],
                frame_buffer_size=FBS, use_controlnet=True,
                controlnet_processor="canny", canny_low=THR[0],
                canny_high=THR[1], canny_reach=8)
    args.update(kw)
    eng = unzero(StreamDiffusionEngine(EngineConfig(**args)))
    eng.prepare()
    return eng


def run_clone(eng, frame):
    out = eng(frame)
    eng.sync_output()
    return out.clone()


def test_engine_graphs_match_eager_and_controls_need_no_recapture():
    fr = [f.cuda() for f in engine_frames(13, FBS)]
    eng = make_engine()
    run_clone(eng, fr[0])
    assert eng._pipelined and eng._graph is True
    g1, g2 = list(eng._g1), list(eng._g2)
    # capturing advanced the stream-batch state by its warm-up steps: hand
    # both slots out afresh, which is the post-prepare() state an eager
    # engine starts from (and the FIFO rows are zero again)
    eng.reset_slot(0)
    eng.reset_slot(1)
    torch.cuda.synchronize()  # the resets wrote on stream A
    assert not eng._hint_feat_buffer.any()
    eager = make_engine(use_hip_graph=False)
    moved = 0
    for i, f in enumerate(fr[1:7]):
        a, b = run_clone(eng, f), run_clone(eager, f)
        assert torch.equal(a, b), f"graph replay diverged from eager at frame {i}"
        moved += int(i > 0 and not torch.equal(a, prev))
        prev = a
    assert moved > 0
    assert torch.equal(eng._hint_feat_buffer, eager._hint_feat_buffer)

    # thresholds of slot 0 between replays: its frames change once the first
    # frame encoded under them has passed the four stages, slot 1's never
    eng.update_canny(5, 12, slot=0)
    assert eng.slot_controls(0)["canny_low"] == 5
    for i, f in enumerate(fr[7:11]):
        a, b = run_clone(eng, f), run_clone(eager, f)
        assert torch.equal(a[1], b[1]), "slot 1 noticed slot 0's thresholds"
        assert torch.equal(a[0], b[0]) == (i < 3), i
    assert eng._canny_thr.tolist() == [[5, 12], [50, 100]]

    # reset: slot 0 equals a freshly prepared engine's first frame
    eng.reset_slot(0)
    assert eng._canny_thr.tolist() == [[50, 100], [50, 100]]
    fresh = make_engine(use_hip_graph=False)
    assert torch.equal(run_clone(eng, fr[11])[0], run_clone(fresh, fr[11])[0])
    assert torch.equal(run_clone(eng, fr[12])[0], run_clone(fresh, fr[12])[0])

    assert all(x is y for x, y in zip(eng._g1, g1)), "g1 re-captured"
    assert all(x is y for x, y in zip(eng._g2, g2)), "g2 re-captured"
    assert len(eng._g1) == 2 and eng._graph is True


def test_engine_hint_is_the_kernels():
    """The graph runs the HIP kernel on the new frames: the FIFO's newest
    block equals the encoder applied to the torch path's hint."""
    fr = [f.cuda() for f in engine_frames(2, FBS)]
    eng = make_engine()
    for f in fr:
        run_clone(eng, f)
    torch.cuda.synchronize()
    hint = reference(fr[-1].cpu(), THR, 8).cuda()
    with torch.no_grad():
        want = eng.controlnet.hint_encoder(hint)
    assert torch.equal(eng._hint_feat_buffer[:FBS], want)
