"""Any-resolution ingest on the GPU: the fit_resize_u8 HIP kernel and the
graph engines fed frames of other resolutions.

The float64 oracle, the cases and the acceptance rule (<= 1 LSB, <= 5 % of
values differing, identity bit-exact) are the ones of tests/test_fit_cpu.py.
"""
import pytest
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import sd_turbo_config
from ai_rtc_agent_amd.engine import StreamDiffusionEngine

from test_fit_cpu import (FIT_CASES, assert_fit_close, case_id, case_ref,
                          noise, oracle_fit)

pytestmark = pytest.mark.gpu

# beyond the shared list: destinations wider than one 64-pixel tile column
# and not a multiple of it, 1-pixel source extents, a column-shaped source
# whose vertical taps span several LDS row chunks, and the webcam case
GPU_CASES = FIT_CASES + [
    ((97, 211), (40, 150), "cover"),
    ((97, 211), (40, 150), "contain"),
    ((1, 7), (16, 24), "stretch"),
    ((5, 3), (9, 70), "contain"),
    ((300, 20), (24, 130), "stretch"),
    ((720, 1280), (512, 512), "cover"),
]


@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_fit_kernel_matches_oracle(case):
    (hs, ws), (h, w), mode = case
    src, ref = case_ref(case)
    out = torch.full((2, h, w, 3), 0xAB, dtype=torch.uint8, device="cuda")
    ops.fit_frame_u8(src.cuda(), out, 1, mode)
    if (hs, ws) == (h, w):
        assert torch.equal(out[1].cpu(), src), "equal sizes must be an exact copy"
    else:
        assert_fit_close(out[1], ref, case_id(case))
    assert bool((out[0] == 0xAB).all())


def test_fit_kernel_slot_isolation_and_bars():
    src = noise(90, 160, seed=5).clamp_(min=1)
    out = torch.full((3, 32, 32, 3), 0xAB, dtype=torch.uint8, device="cuda")
    ops.fit_frame_u8(src.cuda(), out, 1, "contain")
    _, (oy, ox, oh, ow) = ops.fit_geometry(90, 160, 32, 32, "contain")
    got = out.cpu()
    assert bool((got[1, :oy] == 0).all()) and bool((got[1, oy + oh:] == 0).all())
    assert_fit_close(got[1], oracle_fit(src, 32, 32, "contain"), "contain 32x32")
    assert bool((got[0] == 0xAB).all()) and bool((got[2] == 0xAB).all())


def test_fit_kernel_non_contiguous_source():
    big = noise(90, 158, seed=6)
    view = big[::2, 1::2]  # (45, 79, 3), strided in both axes
    assert not view.is_contiguous()
    out = torch.zeros((1, 32, 32, 3), dtype=torch.uint8, device="cuda")
    ops.fit_frame_u8(big.cuda()[::2, 1::2], out, 0, "cover")
    assert_fit_close(out[0], oracle_fit(view.contiguous(), 32, 32, "cover"),
                     "strided view")


@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_fit_kernel_matches_cpu_path(case):
    (hs, ws), (h, w), mode = case
    src, _ = case_ref(case)
    cpu = torch.zeros((1, h, w, 3), dtype=torch.uint8)
    ops.fit_frame_u8(src, cpu, 0, mode)
    gpu = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    ops.fit_frame_u8(src.cuda(), gpu, 0, mode)
    if (hs, ws) == (h, w):
        assert torch.equal(gpu.cpu(), cpu)
    else:
        assert_fit_close(gpu[0], cpu[0], "hip vs cpu " + case_id(case))


# ---------------------------------------------------------------------------
# graph engines (SD-Turbo 512x512 1-step: the smallest config
# tests/test_engine_gpu.py runs)
# ---------------------------------------------------------------------------
MIXED_SIZES = [(360, 640), (600, 450)]


def _run(e, f):
    out = e(f)
    e.sync_output()
    return out.clone()


@pytest.fixture(scope="module")
def mixed_run():
    """One pipelined and one sequential graph engine fed the same sequence:
    an engine-sized frame, 8 frames alternating between two other sizes
    (distinct content each), the engine-sized frame again. The reference for
    the engine-sized frame comes from the sequential engine BEFORE it has
    seen any other size. CPU frames, as the media plane delivers them."""
    eng = {}
    for overlap in (False, True):
        cfg = sd_turbo_config(device="cuda", use_hip_graph=True)
        cfg.pipeline_overlap = overlap
        eng[overlap] = StreamDiffusionEngine(cfg)
        eng[overlap].prepare()
    same = noise(512, 512, seed=99)
    mixed = [noise(*MIXED_SIZES[i % 2], seed=200 + i) for i in range(8)]
    res = {"mixed_frames": mixed}
    for overlap, e in eng.items():
        r = {"before": _run(e, same)}
        if overlap:
            # pairs go in back to back, nothing waits in between: the
            # caller's stream runs ahead of the engine's streams as it does
            # in serving. The first output of a pair has to outlive the
            # second call: only the parity-0 output buffer does (graph 1 of
            # the decode pair shares graph 0's memory pool, so a replay of
            # graph 0 may scribble over graph 1's output) — start on parity 0
            if e._pp:
                _run(e, same)
            r["mixed"] = []
            for i in range(0, 8, 2):
                o0, o1 = e(mixed[i]), e(mixed[i + 1])
                e.sync_output()
                r["mixed"] += [o0.clone(), o1.clone()]
        else:
            r["mixed"] = [_run(e, f) for f in mixed]
        r["slot_after_mixed"] = e._frame_in.clone()
        r["after"] = _run(e, same)
        r["ingest"] = e.stats()["ingest"]
        res[overlap] = r
    return res


def test_mixed_sizes_pipelined_equals_sequential(mixed_run):
    seq, pipe = mixed_run[False], mixed_run[True]
    for i, (a, b) in enumerate(zip(seq["mixed"], pipe["mixed"])):
        assert a.shape == (512, 512, 3)
        assert torch.equal(a, b), f"pipelined diverged at mixed-size frame {i}"
    # distinct inputs gave distinct outputs (no stale slot was replayed)
    for i in range(1, 8):
        assert not torch.equal(pipe["mixed"][i], pipe["mixed"][i - 1])
    # the slot holds the fit of the LAST mixed frame, in both modes
    ref = oracle_fit(mixed_run["mixed_frames"][-1], 512, 512, "cover")
    for r in (seq, pipe):
        assert_fit_close(r["slot_after_mixed"][0], ref, "engine input slot")
    assert pipe["ingest"]["last_source_size"] == [[512, 512]]


def test_engine_sized_frame_unaffected_by_mixed_sizes(mixed_run):
    ref = mixed_run[False]["before"]  # engine that had seen no other size yet
    for overlap in (False, True):
        assert torch.equal(mixed_run[overlap]["before"], ref)
        assert torch.equal(mixed_run[overlap]["after"], ref), (
            f"overlap={overlap}: engine-sized frame changed after mixed sizes")
