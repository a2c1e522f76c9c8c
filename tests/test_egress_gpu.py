"""Any-resolution egress on the GPU: fit_resize_u8 as the RGB egress, the
fused fit_resize_u8_i420 kernel, and graph engines with
output_size == "source".

The float64 oracle, the cases and the acceptance rule (<= 1 LSB, <= 5 % of
values differing, equal sizes bit-exact) are the ones of
tests/test_egress_cpu.py. The I420 kernel is held to more: bit for bit the
colour kernel applied to the RGB kernel's output.
"""
import pytest
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import sd_turbo_config
from ai_rtc_agent_amd.engine import StreamDiffusionEngine

from test_egress_cpu import (EGRESS_CASES, case_id, case_ref)
from test_fit_cpu import assert_fit_close, noise

pytestmark = pytest.mark.gpu

# the webcam case: a 512x512 engine frame back to 720p, bars cut away
GPU_CASES = EGRESS_CASES + [((512, 512), (720, 1280), "contain")]

# I420 targets beyond the cases' own (floored to even): Ht/2 odd (90x160:
# the chroma planes' rows do not line up with the (Ht/2, Wt) tail), and a
# width that is no multiple of 64 or 128 (96x210)
I420_EXTRA = [
    ((64, 64), (0, 0, 64, 64), (90, 160)),
    ((64, 64), (3, 5, 40, 51), (96, 210)),
    ((40, 150), (0, 0, 40, 150), (10, 2)),
    ((40, 150), (7, 11, 30, 100), (2, 300)),
]

GUARD = 0xAB


def _guarded(shape):
    """A destination inside a larger pre-filled buffer: (buffer, view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2048,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[1024:1024 + n].view(shape)


def _assert_guard_intact(buf, n):
    assert bool((buf[:1024] == GUARD).all()), "wrote in front of the destination"
    assert bool((buf[1024 + n:] == GUARD).all()), "wrote past the destination"


@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_rgb_egress_matches_oracle_and_cpu_path(case):
    img, window, size, ref = case_ref(case)
    buf, out = _guarded((*size, 3))
    assert ops.unfit_frame_u8(img.cuda(), window, size, out=out) is out
    _assert_guard_intact(buf, out.numel())
    cpu = ops.unfit_frame_u8(img, window, size)
    if (window[2], window[3]) == size:
        ry, rx, rh, rw = window
        assert torch.equal(out.cpu(), img[ry:ry + rh, rx:rx + rw])
        assert torch.equal(out.cpu(), cpu)
    else:
        assert_fit_close(out, ref, case_id(case))
        assert_fit_close(out, cpu, "hip vs cpu " + case_id(case))
    # the allocating form gives the same bytes
    assert torch.equal(ops.unfit_frame_u8(img.cuda(), window, size), out)


def _check_fused_i420(img, window, size):
    dev = img.cuda()
    rgb = ops.unfit_frame_u8(dev, window, size, fmt="rgb")
    two_launch = ops.rgb_u8_to_i420(rgb)
    fused = ops.unfit_frame_u8(dev, window, size, fmt="i420")
    assert fused.shape == (size[0] // 2 * 3, size[1]) and fused.is_contiguous()
    assert torch.equal(fused, two_launch), "fused I420 != colour kernel of RGB egress"
    buf, out = _guarded(tuple(fused.shape))
    assert ops.unfit_frame_u8(dev, window, size, fmt="i420", out=out) is out
    _assert_guard_intact(buf, out.numel())
    assert torch.equal(out, fused)
    return fused


@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_fused_i420_equals_rgb_egress_then_colour_kernel(case):
    img, window, size, _ = case_ref(case, even=True)
    _check_fused_i420(img, window, size)
    # the RGB it converts is the CPU path's to within the resize's tolerance
    cpu_rgb = ops.unfit_frame_u8(img, window, size, fmt="rgb")
    gpu_rgb = ops.unfit_frame_u8(img.cuda(), window, size, fmt="rgb")
    assert_fit_close(gpu_rgb, cpu_rgb, "hip vs cpu " + case_id(case))


@pytest.mark.parametrize("shape,window,size", I420_EXTRA,
                         ids=lambda v: "x".join(map(str, v)))
def test_fused_i420_plane_layout_edges(shape, window, size):
    _check_fused_i420(noise(*shape, seed=shape[0] * 1000 + shape[1]), window, size)


def test_i420_rejects_odd_sizes_and_bad_out():
    img = noise(16, 24, seed=3).cuda()
    for bad in [(21, 30), (20, 31)]:
        with pytest.raises(ValueError):
            ops.unfit_frame_u8(img, (0, 0, 16, 24), bad, fmt="i420")
    with pytest.raises(ValueError):
        ops.unfit_frame_u8(img, (0, 0, 16, 24), (20, 30), fmt="i420",
                           out=torch.zeros((20, 30), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.unfit_frame_u8(img, (0, 0, 17, 24), (20, 30))
    with pytest.raises(ValueError):
        ops.unfit_frame_u8(img, (0, 0, 16, 24), (20, 30),
                           out=torch.zeros((20, 30, 3), dtype=torch.uint8))


# ---------------------------------------------------------------------------
# graph engines (SD-Turbo 512x512 1-step, the config tests/test_fit_gpu.py
# runs), fed that file's mixed_run sequence
# ---------------------------------------------------------------------------
MIXED_SIZES = [(360, 640), (600, 450)]
COVER_TARGETS = [(360, 360), (450, 450)]


def _engine(overlap, **kw):
    cfg = sd_turbo_config(device="cuda", use_hip_graph=True, **kw)
    cfg.pipeline_overlap = overlap
    e = StreamDiffusionEngine(cfg)
    e.prepare()
    return e


def _run(e, f):
    out = e(f)
    e.sync_output()
    return out.clone()


def _sequence(e, same, mixed, pairs):
    """before / 8 mixed / after, as test_fit_gpu.py's mixed_run feeds them.
    `pairs`: back to back in twos with sync_output() afterwards (the
    caller's stream runs ahead of the engine's streams, as in serving)."""
    r = {"before": _run(e, same)}
    if pairs:
        if e._pp:  # start on parity 0, as that fixture does
            _run(e, same)
        r["mixed"] = []
        for i in range(0, 8, 2):
            o0, o1 = e(mixed[i]), e(mixed[i + 1])
            e.sync_output()
            r["mixed"] += [o0.clone(), o1.clone()]
    else:
        r["mixed"] = [_run(e, f) for f in mixed]
    r["after"] = _run(e, same)
    r["stats"] = e.stats()
    return r


@pytest.fixture(scope="module")
def frames():
    same = noise(512, 512, seed=99)
    mixed = [noise(*MIXED_SIZES[i % 2], seed=200 + i) for i in range(8)]
    return same, mixed


@pytest.fixture(scope="module")
def engine_mode_run(frames):
    """The reference: an "engine"-mode sequential graph engine (RGB)."""
    return _sequence(_engine(False), *frames, pairs=False)


@pytest.fixture(scope="module")
def source_runs(frames):
    return {overlap: _sequence(_engine(overlap, output_size="source"),
                               *frames, pairs=overlap)
            for overlap in (False, True)}


def test_source_size_engines_return_cover_targets(source_runs):
    for overlap, r in source_runs.items():
        for i, o in enumerate(r["mixed"]):
            assert o.shape == (*COVER_TARGETS[i % 2], 3), (overlap, i, o.shape)
            assert o.dtype == torch.uint8
        assert r["before"].shape == (512, 512, 3)
        assert r["stats"]["egress"] == {
            "output_size": "source", "max_side": 0,
            "last_output_size": [[512, 512]]}


def test_source_size_pipelined_equals_sequential(source_runs):
    seq, pipe = source_runs[False], source_runs[True]
    for i, (a, b) in enumerate(zip(seq["mixed"], pipe["mixed"])):
        assert torch.equal(a, b), f"pipelined diverged at mixed-size frame {i}"
    for i in range(2, 8):  # distinct inputs gave distinct outputs
        assert not torch.equal(pipe["mixed"][i], pipe["mixed"][i - 2])


def test_source_size_is_the_egress_of_the_engine_mode_output(
        source_runs, engine_mode_run):
    """The egress read the FINISHED frame (stream-B ordering): every output
    is ops.unfit_frame_u8 of what an "engine"-mode engine returns."""
    for i, full in enumerate(engine_mode_run["mixed"]):
        assert full.shape == (512, 512, 3)
        window, size = ops.unfit_geometry(*MIXED_SIZES[i % 2], 512, 512, "cover")
        assert (window, size) == ((0, 0, 512, 512), COVER_TARGETS[i % 2])
        ref = ops.unfit_frame_u8(full, window, size)
        for overlap, r in source_runs.items():
            assert torch.equal(r["mixed"][i], ref), (overlap, i)


def test_engine_sized_frame_same_bytes_in_both_modes(source_runs, engine_mode_run):
    ref = engine_mode_run["before"]
    assert torch.equal(engine_mode_run["after"], ref)
    for overlap, r in source_runs.items():
        assert torch.equal(r["before"], ref), overlap
        assert torch.equal(r["after"], ref), (
            f"overlap={overlap}: engine-sized frame changed after mixed sizes")


@pytest.fixture(scope="module")
def i420_runs(frames):
    """The pipelined source-size engine with output_format="i420" over the
    same sequence, and the engine-sized frame through the "engine"-mode
    I420 graph."""
    same, mixed = frames
    r = _sequence(_engine(True, output_size="source", output_format="i420"),
                  same, mixed, pairs=True)
    r["engine_mode"] = _run(_engine(True, output_format="i420"), same)
    return r


def test_source_size_i420_pipelined(i420_runs, engine_mode_run):
    """output_format="i420": the graph stays the RGB one and the egress
    writes planes; engine-sized frames equal the "engine"-mode I420 graph."""
    r, eng_i420 = i420_runs, i420_runs["engine_mode"]
    assert eng_i420.shape == (768, 512)
    assert torch.equal(r["before"], eng_i420)
    assert torch.equal(r["after"], eng_i420)
    assert torch.equal(eng_i420, ops.rgb_u8_to_i420(engine_mode_run["before"]))
    for i, (o, full) in enumerate(zip(r["mixed"], engine_mode_run["mixed"])):
        ht, wt = COVER_TARGETS[i % 2]
        assert o.shape == (ht // 2 * 3, wt), (i, o.shape)
        ref = ops.rgb_u8_to_i420(
            ops.unfit_frame_u8(full, (0, 0, 512, 512), (ht, wt)))
        assert torch.equal(o, ref), f"I420 egress diverged at mixed-size frame {i}"
