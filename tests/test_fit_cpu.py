"""Any-resolution ingest (ops.fit_geometry / ops.fit_frame_u8) — CPU tests.

The oracle below is independent of `ops`: integer geometry re-derived from
the definition, dense per-axis weight matrices of the antialiased triangle
filter in float64, applied with einsum, rounded half-to-even and placed in
the destination window. tests/test_fit_gpu.py imports it for the HIP kernel.

Acceptance for every comparison against it: max |diff| <= 1 LSB and at most
5 % of values differ (float64 vs f32 accumulation only moves rounding ties;
the oracle-vs-torch figure on these shapes is <= 1.92 %). Identity cases
are bit-exact.
"""
import asyncio

import numpy as np
import pytest
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import EngineConfig
from ai_rtc_agent_amd.engine import StreamDiffusionEngine

MODES = ("cover", "contain", "stretch")

# (Hs, Ws) -> (H, W), mode
FIT_CASES = [
    ((48, 64), (32, 32), "cover"),
    ((45, 79), (32, 32), "cover"),
    ((90, 160), (64, 64), "cover"),
    ((90, 160), (64, 64), "contain"),
    ((90, 160), (64, 64), "stretch"),
    ((37, 53), (64, 64), "cover"),      # upscale
    ((64, 64), (64, 64), "cover"),      # exact
    ((200, 360), (32, 32), "cover"),    # 6.25x downscale, many taps
    ((33, 47), (16, 24), "cover"),
]


# ---------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------
def _rdiv(a, b, c):
    return max(1, (a * b + c // 2) // c)


def oracle_geometry(Hs, Ws, H, W, mode):
    if mode == "cover":
        if Ws * H > Hs * W:
            ch, cw = Hs, _rdiv(Hs, W, H)
        else:
            cw, ch = Ws, _rdiv(Ws, H, W)
        return ((Hs - ch) // 2, (Ws - cw) // 2, ch, cw), (0, 0, H, W)
    if mode == "contain":
        if Ws * H > Hs * W:
            ow, oh = W, _rdiv(W, Hs, Ws)
        else:
            oh, ow = H, _rdiv(H, Ws, Hs)
        return (0, 0, Hs, Ws), ((H - oh) // 2, (W - ow) // 2, oh, ow)
    assert mode == "stretch"
    return (0, 0, Hs, Ws), (0, 0, H, W)


def axis_weights(n_in, n_out):
    """(n_out, n_in) float64 weights of the antialiased triangle filter."""
    scale = n_in / n_out
    sup = max(scale, 1.0)
    m = np.zeros((n_out, n_in), dtype=np.float64)
    for o in range(n_out):
        c = (o + 0.5) * scale
        lo = max(int(c - sup + 0.5), 0)
        hi = min(int(c + sup + 0.5), n_in)
        j = np.arange(lo, hi, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((j - c + 0.5) / sup))
        m[o, lo:hi] = w / w.sum()
    return m


def oracle_fit(src, H, W, mode):
    """src (Hs, Ws, 3) u8 tensor -> (H, W, 3) u8 tensor."""
    a = src.numpy().astype(np.float64)
    (y0, x0, ch, cw), (oy, ox, oh, ow) = oracle_geometry(
        a.shape[0], a.shape[1], H, W, mode)
    win = a[y0:y0 + ch, x0:x0 + cw]
    # rows, then columns: one three-operand einsum is evaluated as a single
    # naive loop nest, hours at webcam sizes
    res = np.einsum("oy,yxc->oxc", axis_weights(ch, oh), win)
    res = np.einsum("px,oxc->opc", axis_weights(cw, ow), res)
    out = np.zeros((H, W, 3), dtype=np.uint8)
    out[oy:oy + oh, ox:ox + ow] = np.clip(np.rint(res), 0, 255).astype(np.uint8)
    return torch.from_numpy(out)


def noise(h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)


def assert_fit_close(got, ref, what=""):
    """<= 1 LSB everywhere and <= 5 % of values different."""
    d = (got.cpu().int() - ref.int()).abs()
    mx, frac = int(d.max()), float((d != 0).float().mean())
    print(f"{what}: max|diff|={mx} differing={100 * frac:.2f}%")
    assert mx <= 1, f"{what}: max abs diff {mx} LSB"
    assert frac <= 0.05, f"{what}: {100 * frac:.2f}% of values differ"


_ORACLE_CACHE = {}


def case_ref(case):
    """(src, oracle result) for a FIT_CASES entry, computed once."""
    if case not in _ORACLE_CACHE:
        (hs, ws), (h, w), mode = case
        src = noise(hs, ws, seed=hs * 1000 + ws)
        _ORACLE_CACHE[case] = (src, oracle_fit(src, h, w, mode))
    return _ORACLE_CACHE[case]


def case_id(case):
    (hs, ws), (h, w), mode = case
    return f"{hs}x{ws}-to-{h}x{w}-{mode}"


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dst", [(512, 512), (256, 512)])
@pytest.mark.parametrize("src", [(720, 1280), (1280, 720), (480, 640),
                                 (600, 600), (1, 1000), (1000, 1), (3, 5)])
@pytest.mark.parametrize("mode", MODES)
def test_fit_geometry_windows(src, dst, mode):
    (Hs, Ws), (H, W) = src, dst
    (y0, x0, ch, cw), (oy, ox, oh, ow) = ops.fit_geometry(Hs, Ws, H, W, mode)
    assert ((y0, x0, ch, cw), (oy, ox, oh, ow)) == oracle_geometry(Hs, Ws, H, W, mode)
    # in range and never empty
    assert ch >= 1 and cw >= 1 and oh >= 1 and ow >= 1
    assert 0 <= y0 and y0 + ch <= Hs and 0 <= x0 and x0 + cw <= Ws
    assert 0 <= oy and oy + oh <= H and 0 <= ox and ox + ow <= W
    # centred (floor division puts the odd pixel after the window)
    assert y0 == (Hs - ch) // 2 and x0 == (Ws - cw) // 2
    assert oy == (H - oh) // 2 and ox == (W - ow) // 2
    if mode == "cover":
        assert (oy, ox, oh, ow) == (0, 0, H, W)
        assert ch == Hs or cw == Ws  # the LARGEST window of that aspect
    else:
        assert (y0, x0, ch, cw) == (0, 0, Hs, Ws)
    if mode == "contain":
        assert oh == H or ow == W
    if mode == "stretch":
        assert (oy, ox, oh, ow) == (0, 0, H, W)


def test_fit_geometry_known_values():
    # 16:9 webcam into the square engine: centred 720x720 crop
    assert ops.fit_geometry(720, 1280, 512, 512, "cover") == (
        (0, 280, 720, 720), (0, 0, 512, 512))
    # ... or letterboxed: 512 * 720/1280 = 288 rows, 112 black above/below
    assert ops.fit_geometry(720, 1280, 512, 512, "contain") == (
        (0, 0, 720, 1280), (112, 0, 288, 512))
    # portrait phone into 2:1
    assert ops.fit_geometry(1280, 720, 256, 512, "cover") == (
        (460, 0, 360, 720), (0, 0, 256, 512))
    assert ops.fit_geometry(1280, 720, 256, 512, "contain") == (
        (0, 0, 1280, 720), (0, 184, 256, 144))
    with pytest.raises(ValueError):
        ops.fit_geometry(4, 4, 4, 4, "fill")
    with pytest.raises(ValueError):
        ops.fit_geometry(0, 4, 4, 4, "cover")


# ---------------------------------------------------------------------------
# fit_frame_u8, CPU path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", FIT_CASES, ids=case_id)
def test_fit_frame_cpu_matches_oracle(case):
    (hs, ws), (h, w), mode = case
    src, ref = case_ref(case)
    out = torch.full((2, h, w, 3), 0xAB, dtype=torch.uint8)
    ops.fit_frame_u8(src, out, 1, mode)
    if (hs, ws) == (h, w):
        assert torch.equal(out[1], src), "equal sizes must be an exact copy"
        assert torch.equal(out[1], ref)
    else:
        assert_fit_close(out[1], ref, case_id(case))
    assert bool((out[0] == 0xAB).all())


def test_contain_bars_are_zero_and_only_the_slot_changes():
    src = noise(90, 160, seed=5).clamp_(min=1)  # no zeros inside the picture
    out = torch.full((3, 32, 32, 3), 0xAB, dtype=torch.uint8)
    ops.fit_frame_u8(src, out, 1, "contain")
    _, (oy, ox, oh, ow) = ops.fit_geometry(90, 160, 32, 32, "contain")
    assert (oy, ox, oh, ow) == (7, 0, 18, 32)
    assert bool((out[1, :oy] == 0).all()) and bool((out[1, oy + oh:] == 0).all())
    assert bool((out[1, oy:oy + oh] != 0).any())
    assert_fit_close(out[1], oracle_fit(src, 32, 32, "contain"), "contain 32x32")
    assert bool((out[0] == 0xAB).all()) and bool((out[2] == 0xAB).all())


def test_fit_frame_rejects_bad_arguments():
    out = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    src = noise(4, 6)
    with pytest.raises(IndexError):
        ops.fit_frame_u8(src, out, 2)
    with pytest.raises(TypeError):
        ops.fit_frame_u8(src.float(), out, 0)
    with pytest.raises(ValueError):
        ops.fit_frame_u8(src[None], out, 0)
    with pytest.raises(ValueError):
        ops.fit_frame_u8(src, out, 0, "fill")


# ---------------------------------------------------------------------------
# engine + serving layers (tiny CPU engine, 64x64)
# ---------------------------------------------------------------------------
def make_engine(cfg, **kw):
    for k, v in kw.items():
        setattr(cfg, k, v)
    e = StreamDiffusionEngine(cfg)
    e.prepare()
    return e


def test_fit_mode_config_default_and_env(monkeypatch):
    monkeypatch.delenv("AIRTC_FIT_MODE", raising=False)
    assert EngineConfig().fit_mode == "cover"
    monkeypatch.setenv("AIRTC_FIT_MODE", "contain")
    assert EngineConfig().fit_mode == "contain"
    assert EngineConfig(fit_mode="stretch").fit_mode == "stretch"
    with pytest.raises(ValueError):
        make_engine(EngineConfig(model_family="tiny", width=64, height=64,
                                 device="cpu", use_hip_graph=False,
                                 use_lcm_lora=False, fit_mode="fill"))


def test_engine_accepts_other_resolutions(tiny_cfg):
    e = make_engine(tiny_cfg)
    assert e.stats()["ingest"]["fit_mode"] == "cover"
    out = e(noise(48, 80, seed=1))
    assert out.shape == (64, 64, 3) and out.dtype == torch.uint8
    assert e.stats()["ingest"]["last_source_size"] == [[48, 80]]
    # what the engine saw is the fitted frame
    assert_fit_close(e._frame_in[0], oracle_fit(noise(48, 80, seed=1), 64, 64, "cover"),
                     "engine input slot")
    out = e(noise(96, 64, seed=2))  # resolution changes mid-session
    assert out.shape == (64, 64, 3) and out.dtype == torch.uint8
    assert e.stats()["ingest"]["last_source_size"] == [[96, 64]]
    out = e(noise(64, 64, seed=3))
    assert e.stats()["ingest"]["last_source_size"] == [[64, 64]]


def test_engine_batch_of_differing_sizes(tiny_cfg):
    e = make_engine(tiny_cfg, frame_buffer_size=2, fit_mode="contain")
    frames = [noise(48, 80, seed=1), noise(64, 64, seed=2)]
    out = e(frames)
    assert out.shape == (2, 64, 64, 3)
    assert e.stats()["ingest"] == {
        "fit_mode": "contain", "engine_size": [64, 64],
        "last_source_size": [[48, 80], [64, 64]]}
    assert_fit_close(e._frame_in[0], oracle_fit(frames[0], 64, 64, "contain"), "slot 0")
    assert torch.equal(e._frame_in[1], frames[1]), "engine-sized slot is a plain copy"
    # one (fbs, Hs, Ws, 3) tensor of another size works too
    out = e(torch.stack([noise(30, 50, seed=3), noise(30, 50, seed=4)]))
    assert out.shape == (2, 64, 64, 3)
    assert e.stats()["ingest"]["last_source_size"] == [[30, 50], [30, 50]]
    with pytest.raises(ValueError):
        e([frames[0]])


def test_similarity_filter_sees_the_fitted_frame(tiny_cfg):
    tiny_cfg.similarity_filter.enabled = True
    e = make_engine(tiny_cfg)
    seen = []
    real = e.sim_filter.should_skip
    e.sim_filter.should_skip = lambda x: (seen.append(tuple(x.shape)), real(x))[1]
    f = noise(48, 80, seed=1)
    for _ in range(3):
        out = e(f)
    assert out.shape == (64, 64, 3)
    assert seen and all(s == (1, 64, 64, 3) for s in seen)


def test_engine_sized_frames_ignore_fit_mode():
    outs = []
    for mode in MODES:
        cfg = EngineConfig(model_family="tiny", width=64, height=64,
                           device="cpu", acceleration="eager",
                           use_hip_graph=False, use_lcm_lora=False,
                           fit_mode=mode)
        e = make_engine(cfg)
        outs.append([e(noise(64, 64, seed=10 + i)).clone() for i in range(2)])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


def test_batched_pipeline_mixed_resolutions(tiny_cfg, tmp_path, monkeypatch):
    from ai_rtc_agent_amd.parallel.batching import BatchedPipeline
    from ai_rtc_agent_amd.pipeline import StreamDiffusionPipeline

    monkeypatch.setenv("ENGINES_CACHE", str(tmp_path))
    tiny_cfg.frame_buffer_size = 2
    base = StreamDiffusionPipeline(cfg=tiny_cfg)

    async def body():
        bp = BatchedPipeline(base, 2)
        a, b = bp.acquire("s-a"), bp.acquire("s-b")
        ra, rb = await asyncio.gather(a(noise(48, 80, seed=1)),
                                      b(noise(64, 64, seed=2)))
        assert ra.shape == (64, 64, 3) and rb.shape == (64, 64, 3)
        assert ra.dtype == torch.uint8 and rb.dtype == torch.uint8
        st = bp.stats()
        assert st["ingest"]["last_source_size"][a.slot] == [48, 80]
        assert st["ingest"]["last_source_size"][b.slot] == [64, 64]
        # a lone publisher at another size next to a slot that has gone quiet
        rc = await a(noise(96, 64, seed=3))
        assert rc.shape == (64, 64, 3)
        bp.release("s-a")
        bp.release("s-b")

    loop = asyncio.new_event_loop()
    try:
        loop.run_until_complete(asyncio.wait_for(body(), 120))
    finally:
        loop.close()
