"""Any-resolution egress (ops.unfit_geometry / ops.unfit_frame_u8 and
EngineConfig.output_size == "source") — CPU tests.

The oracle is independent of `ops`: the read window and the target size are
re-derived here from tests/test_fit_cpu.py's oracle_geometry, and the resize
is that file's dense float64 weight matrices applied with einsum and rounded
half-to-even. tests/test_egress_gpu.py imports it for the HIP kernels.

Acceptance against it is the fit rule (assert_fit_close): max |diff| <= 1 LSB
and at most 5 % of values differing; float64 vs f32 accumulation only moves
rounding ties (the oracle-vs-torch figure on these cases is <= 0.74 %).
Equal-size cases are bit-exact, and I420 is exactly the integer colour
conversion of the RGB result.
"""
import asyncio

import numpy as np
import pytest
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import EngineConfig
from ai_rtc_agent_amd.engine import StreamDiffusionEngine
from ai_rtc_agent_amd.ops.interface import _rgb_u8_to_i420_ref

from test_fit_cpu import (MODES, assert_fit_close, axis_weights, noise,
                          oracle_geometry)

# (engine H, W) <- (source Hs, Ws), mode
EGRESS_CASES = [
    ((64, 64), (90, 160), "cover"),
    ((64, 64), (90, 160), "contain"),
    ((64, 64), (90, 160), "stretch"),
    ((32, 32), (45, 79), "cover"),        # odd target 45x45; I420 at 44x44
    ((64, 64), (37, 53), "cover"),        # egress that downsizes
    ((16, 24), (33, 47), "cover"),
    ((32, 32), (200, 360), "contain"),    # 18-row window upscaled 11x
    ((40, 150), (97, 211), "cover"),      # wider than one 64-pixel tile
    ((40, 150), (97, 211), "contain"),    # window with rx > 0
    ((24, 130), (300, 20), "stretch"),    # 300 rows x 20 columns
    ((16, 24), (1, 7), "stretch"),
    ((9, 70), (5, 3), "contain"),
    ((64, 64), (64, 64), "cover"),        # identity
]


# ---------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------
def oracle_unfit_geometry(Hs, Ws, H, W, mode, even=False, max_side=0):
    (_, _, ch, cw), dst = oracle_geometry(Hs, Ws, H, W, mode)
    if mode == "contain":
        window, (ht, wt) = dst, (Hs, Ws)
    elif mode == "cover":
        window, (ht, wt) = (0, 0, H, W), (ch, cw)
    else:
        window, (ht, wt) = (0, 0, H, W), (Hs, Ws)
    m = max(ht, wt)
    if max_side > 0 and m > max_side:
        ht = max(1, (ht * max_side + m // 2) // m)
        wt = max(1, (wt * max_side + m // 2) // m)
    if even:
        ht, wt = max(2, ht // 2 * 2), max(2, wt // 2 * 2)
    return window, (ht, wt)


def oracle_unfit(img, window, size):
    """img (H, W, 3) u8 tensor -> (Ht, Wt, 3) u8 tensor, float64."""
    ry, rx, rh, rw = window
    ht, wt = size
    win = img.numpy().astype(np.float64)[ry:ry + rh, rx:rx + rw]
    res = np.einsum("oy,yxc->oxc", axis_weights(rh, ht), win)
    res = np.einsum("px,oxc->opc", axis_weights(rw, wt), res)
    return torch.from_numpy(np.clip(np.rint(res), 0, 255).astype(np.uint8))


def case_id(case):
    (h, w), (hs, ws), mode = case
    return f"{h}x{w}-back-to-{hs}x{ws}-{mode}"


_CACHE = {}


def case_ref(case, even=False):
    """(engine frame, window, target size, oracle result), computed once."""
    key = (case, even)
    if key not in _CACHE:
        (h, w), (hs, ws), mode = case
        img = noise(h, w, seed=h * 1000 + w)
        window, size = oracle_unfit_geometry(hs, ws, h, w, mode, even=even)
        _CACHE[key] = (img, window, size, oracle_unfit(img, window, size))
    return _CACHE[key]


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
GEO_SRC = [(720, 1280), (1280, 720), (480, 640), (600, 600), (1, 1000), (3, 5)]
GEO_DST = [(512, 512), (256, 512)]


@pytest.mark.parametrize("dst", GEO_DST)
@pytest.mark.parametrize("src", GEO_SRC)
@pytest.mark.parametrize("mode", MODES)
def test_unfit_geometry_table(src, dst, mode):
    (Hs, Ws), (H, W) = src, dst
    (_, _, ch, cw), (oy, ox, oh, ow) = oracle_geometry(Hs, Ws, H, W, mode)
    window, size = ops.unfit_geometry(Hs, Ws, H, W, mode)
    if mode == "stretch":
        assert (window, size) == ((0, 0, H, W), (Hs, Ws))
    elif mode == "contain":
        assert (window, size) == ((oy, ox, oh, ow), (Hs, Ws))
    else:
        assert (window, size) == ((0, 0, H, W), (ch, cw))
    ry, rx, rh, rw = window
    assert rh >= 1 and rw >= 1 and ry >= 0 and rx >= 0
    assert ry + rh <= H and rx + rw <= W
    assert size[0] >= 1 and size[1] >= 1


@pytest.mark.parametrize("dst", GEO_DST)
@pytest.mark.parametrize("src", GEO_SRC)
@pytest.mark.parametrize("mode", MODES)
def test_unfit_geometry_even_and_max_side(src, dst, mode):
    (Hs, Ws), (H, W) = src, dst
    window, (ht, wt) = ops.unfit_geometry(Hs, Ws, H, W, mode)
    w_even, (he, we) = ops.unfit_geometry(Hs, Ws, H, W, mode, even=True)
    assert w_even == window
    assert (he, we) == (max(2, ht - ht % 2), max(2, wt - wt % 2))
    assert he % 2 == 0 and we % 2 == 0 and he >= 2 and we >= 2
    for cap in (1, 7, 320, 5000):
        w_cap, (hc, wc) = ops.unfit_geometry(Hs, Ws, H, W, mode, max_side=cap)
        assert w_cap == window
        assert (w_cap, (hc, wc)) == oracle_unfit_geometry(
            Hs, Ws, H, W, mode, max_side=cap)
        if max(ht, wt) <= cap:
            assert (hc, wc) == (ht, wt), "the cap never enlarges"
            continue
        assert max(hc, wc) == cap, "the longer side becomes exactly max_side"
        # the shorter side is the rounded scaled value (>= 1): aspect kept
        # to within half a pixel of the scaled size
        lo, s = min(ht, wt), min(hc, wc)
        assert s >= 1 and (s == 1 or abs(s - lo * cap / max(ht, wt)) <= 0.5)
        # both adjustments, in order: cap, then floor to even
        _, (hb, wb) = ops.unfit_geometry(Hs, Ws, H, W, mode, even=True,
                                         max_side=cap)
        assert (hb, wb) == (max(2, hc - hc % 2), max(2, wc - wc % 2))


@pytest.mark.parametrize("mode", MODES)
def test_unfit_geometry_identity_and_errors(mode):
    for h, w in [(512, 512), (256, 512), (9, 70)]:
        assert ops.unfit_geometry(h, w, h, w, mode) == ((0, 0, h, w), (h, w))
    for bad in [(0, 5, 8, 8), (5, 0, 8, 8), (5, 5, 0, 8), (5, 5, 8, -1)]:
        with pytest.raises(ValueError):
            ops.unfit_geometry(*bad, mode)
    with pytest.raises(ValueError):
        ops.unfit_geometry(5, 5, 8, 8, "fill")
    with pytest.raises(ValueError):
        ops.unfit_geometry(5, 5, 8, 8, mode, max_side=-1)


# ---------------------------------------------------------------------------
# op (torch reference path)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", EGRESS_CASES, ids=case_id)
def test_unfit_matches_oracle(case):
    (h, w), (hs, ws), mode = case
    img, window, size, ref = case_ref(case)
    assert (window, size) == ops.unfit_geometry(hs, ws, h, w, mode)
    got = ops.unfit_frame_u8(img, window, size)
    assert got.shape == (*size, 3) and got.dtype == torch.uint8
    assert got.is_contiguous()
    if (window[2], window[3]) == size:
        assert torch.equal(got, img[window[0]:window[0] + window[2],
                                    window[1]:window[1] + window[3]])
        assert got.data_ptr() != img.data_ptr(), "never a view of the input"
    else:
        assert_fit_close(got, ref, case_id(case))


@pytest.mark.parametrize("case", EGRESS_CASES, ids=case_id)
def test_unfit_i420_is_the_conversion_of_rgb(case):
    img, window, size, _ = case_ref(case, even=True)
    rgb = ops.unfit_frame_u8(img, window, size, fmt="rgb")
    yuv = ops.unfit_frame_u8(img, window, size, fmt="i420")
    assert yuv.shape == (size[0] // 2 * 3, size[1]) and yuv.dtype == torch.uint8
    assert torch.equal(yuv, _rgb_u8_to_i420_ref(rgb[None])[0])
    out = torch.full_like(yuv, 0xAB)
    assert ops.unfit_frame_u8(img, window, size, fmt="i420", out=out) is out
    assert torch.equal(out, yuv)


def test_unfit_out_and_bad_arguments():
    img = noise(16, 24, seed=3)
    window, size = (2, 4, 10, 12), (21, 31)
    ref = ops.unfit_frame_u8(img, window, size)
    out = torch.zeros((21, 31, 3), dtype=torch.uint8)
    assert ops.unfit_frame_u8(img, window, size, out=out) is out
    assert torch.equal(out, ref)
    for bad_size in [(21, 30), (20, 31), (1, 2)]:  # odd or too small
        with pytest.raises(ValueError):
            ops.unfit_frame_u8(img, window, bad_size, fmt="i420")
    with pytest.raises(ValueError):
        ops.unfit_frame_u8(img, window, size, fmt="nv12")
    with pytest.raises(ValueError):
        ops.unfit_frame_u8(img, window, size, out=torch.zeros((21, 31), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.unfit_frame_u8(img, window, size, out=torch.zeros((21, 31, 3)))
    with pytest.raises(TypeError):
        ops.unfit_frame_u8(img.float(), window, size)
    with pytest.raises(ValueError):
        ops.unfit_frame_u8(img[None], window, size)
    for bad_window in [(0, 0, 17, 24), (8, 0, 9, 24), (0, -1, 4, 4), (0, 0, 0, 4)]:
        with pytest.raises(ValueError):
            ops.unfit_frame_u8(img, bad_window, size)
    with pytest.raises(ValueError):
        ops.unfit_frame_u8(img, window, (0, 8))


# ---------------------------------------------------------------------------
# engine + serving layers (tiny CPU engine, 64x64)
# ---------------------------------------------------------------------------
def make_engine(cfg, **kw):
    for k, v in kw.items():
        setattr(cfg, k, v)
    e = StreamDiffusionEngine(cfg)
    e.prepare()
    return e


def tiny(**kw):
    base = dict(model_family="tiny", width=64, height=64, device="cpu",
                acceleration="eager", use_hip_graph=False, use_lcm_lora=False)
    base.update(kw)
    return EngineConfig(**base)


def test_output_size_config_default_env_and_validation(monkeypatch):
    monkeypatch.delenv("AIRTC_OUTPUT_SIZE", raising=False)
    monkeypatch.delenv("AIRTC_OUTPUT_MAX_SIDE", raising=False)
    cfg = EngineConfig()
    assert cfg.output_size == "engine" and cfg.output_max_side == 0
    monkeypatch.setenv("AIRTC_OUTPUT_SIZE", "source")
    monkeypatch.setenv("AIRTC_OUTPUT_MAX_SIDE", "960")
    cfg = EngineConfig()
    assert cfg.output_size == "source" and cfg.output_max_side == 960
    assert EngineConfig(output_size="engine").output_size == "engine"
    with pytest.raises(ValueError):
        EngineConfig(output_size="native")
    with pytest.raises(ValueError):
        EngineConfig(output_max_side=-1)


def test_default_config_returns_the_stacked_engine_size(tiny_cfg):
    e = make_engine(tiny_cfg, frame_buffer_size=2)
    out = e([noise(48, 80, seed=1), noise(64, 64, seed=2)])
    assert isinstance(out, torch.Tensor) and out.shape == (2, 64, 64, 3)
    assert "egress" not in e.stats()


def test_single_frame_comes_back_at_its_own_size(tiny_cfg):
    e = make_engine(tiny_cfg, output_size="source")
    out = e(noise(48, 80, seed=1))  # cover: the 48x48 window that was used
    assert isinstance(out, torch.Tensor)
    assert out.shape == (48, 48, 3) and out.dtype == torch.uint8
    assert e.stats()["egress"] == {
        "output_size": "source", "max_side": 0, "last_output_size": [[48, 48]]}
    out = e(noise(96, 64, seed=2))  # resolution changes mid-session
    assert out.shape == (64, 64, 3)
    out = e(noise(200, 120, seed=3))
    assert out.shape == (120, 120, 3)
    assert e.stats()["egress"]["last_output_size"] == [[120, 120]]


def test_batch_comes_back_per_slot_and_contain_has_no_bars(tiny_cfg):
    e = make_engine(tiny_cfg, frame_buffer_size=2, fit_mode="contain",
                    output_size="source")
    ref = make_engine(tiny(frame_buffer_size=2, fit_mode="contain"))
    frames = [noise(45, 80, seed=1), noise(100, 50, seed=2)]
    out, eng_out = e(frames), ref(frames)
    assert isinstance(out, list) and len(out) == 2
    assert out[0].shape == (45, 80, 3) and out[1].shape == (100, 50, 3)
    assert e.stats()["egress"]["last_output_size"] == [[45, 80], [100, 50]]
    # each slot is the egress of what an "engine"-mode engine returns, read
    # from the picture window only: the bars (stylised or not) are cut away
    for b, (hs, ws) in enumerate([(45, 80), (100, 50)]):
        window, size = ops.unfit_geometry(hs, ws, 64, 64, "contain")
        assert window == ops.fit_geometry(hs, ws, 64, 64, "contain")[1]
        assert window != (0, 0, 64, 64)
        assert torch.equal(out[b], ops.unfit_frame_u8(eng_out[b], window, size))
        assert_fit_close(out[b], oracle_unfit(eng_out[b], window, size), f"slot {b}")
    with pytest.raises(ValueError):
        e([frames[0]])


def test_max_side_caps_what_comes_back(tiny_cfg):
    e = make_engine(tiny_cfg, fit_mode="stretch", output_size="source",
                    output_max_side=40)
    assert e(noise(60, 80, seed=1)).shape == (30, 40, 3)
    assert e(noise(20, 30, seed=2)).shape == (20, 30, 3)
    assert e.stats()["egress"]["max_side"] == 40


@pytest.mark.parametrize("fmt", ["rgb", "i420"])
def test_engine_sized_sources_match_engine_mode(fmt):
    outs = {}
    for size in ("engine", "source"):
        e = make_engine(tiny(output_format=fmt, output_size=size))
        outs[size] = [e(noise(64, 64, seed=10 + i)).clone() for i in range(3)]
        assert ("egress" in e.stats()) == (size == "source")
    shape = (64, 64, 3) if fmt == "rgb" else (96, 64)
    for a, b in zip(outs["engine"], outs["source"]):
        assert b.shape == shape
        assert torch.equal(a, b)


def test_i420_source_size_is_even_and_is_the_conversion(tiny_cfg):
    e = make_engine(tiny_cfg, output_format="i420", output_size="source")
    ref = make_engine(tiny())
    f = noise(45, 79, seed=4)  # cover target 45x45 -> 44x44 for I420
    out, eng_out = e(f), ref(f)
    assert out.shape == (66, 44) and ops.is_i420(out)
    rgb = ops.unfit_frame_u8(eng_out, (0, 0, 64, 64), (44, 44))
    assert torch.equal(out, ops.rgb_u8_to_i420(rgb))
    assert e.stats()["egress"]["last_output_size"] == [[44, 44]]


def test_similarity_skip_never_answers_with_the_old_size(tiny_cfg):
    tiny_cfg.similarity_filter.enabled = True
    tiny_cfg.similarity_filter.threshold = 0.5
    e = make_engine(tiny_cfg, fit_mode="stretch", output_size="source")
    e.sim_filter.should_skip = lambda x: True  # a static scene, always skipped
    flat = torch.full((48, 80, 3), 90, dtype=torch.uint8)
    first = e(flat)                       # nothing to skip to yet
    assert first.shape == (48, 80, 3)
    assert e(flat) is first, "same size: the skip returns the previous object"
    other = e(torch.full((30, 50, 3), 90, dtype=torch.uint8))
    assert other.shape == (30, 50, 3), "a size change is never answered with the old size"
    assert e(torch.full((30, 50, 3), 90, dtype=torch.uint8)) is other
    back = e(flat)
    assert back.shape == (48, 80, 3) and back is not first
    # reset_slot: the first call afterwards is never a skip
    e.reset_slot(0)
    assert e.stats()["egress"]["last_output_size"] == [None]
    again = e(flat)
    assert again is not back and again.shape == (48, 80, 3)


def test_batched_pipeline_resolves_each_session_at_its_own_size(
        tiny_cfg, tmp_path, monkeypatch):
    from ai_rtc_agent_amd.parallel.batching import BatchedPipeline
    from ai_rtc_agent_amd.pipeline import StreamDiffusionPipeline

    monkeypatch.setenv("ENGINES_CACHE", str(tmp_path))
    tiny_cfg.frame_buffer_size = 2
    tiny_cfg.fit_mode = "contain"
    tiny_cfg.output_size = "source"
    base = StreamDiffusionPipeline(cfg=tiny_cfg)

    async def body():
        bp = BatchedPipeline(base, 2)
        a, b = bp.acquire("s-a"), bp.acquire("s-b")
        ra, rb = await asyncio.gather(a(noise(72, 128, seed=1)),
                                      b(noise(48, 64, seed=2)))
        assert ra.shape == (72, 128, 3) and rb.shape == (48, 64, 3)
        assert ra.dtype == torch.uint8 and rb.dtype == torch.uint8
        st = bp.stats()
        assert st["egress"]["last_output_size"][a.slot] == [72, 128]
        assert st["egress"]["last_output_size"][b.slot] == [48, 64]
        # a session changes its resolution next to one that has gone quiet
        rc = await a(noise(96, 64, seed=3))
        assert rc.shape == (96, 64, 3)
        bp.release("s-a")
        bp.release("s-b")

    loop = asyncio.new_event_loop()
    try:
        loop.run_until_complete(asyncio.wait_for(body(), 120))
    finally:
        loop.close()


def test_size_change_reaches_the_encoder_as_a_new_size_keyframe(tiny_cfg):
    """The agent's encoder sees whatever size the engine returns: when a
    session changes resolution mid-stream, H264SwCodec re-creates its
    encoder and the first frame at the new size is an IDR that a decoder
    which has seen nothing yet can open, at the new size."""
    from ai_rtc_agent_amd.config import EncoderConfig
    from ai_rtc_agent_amd.media.codec import H264SwCodec

    e = make_engine(tiny_cfg, fit_mode="stretch", output_size="source")
    enc = H264SwCodec(EncoderConfig(), keyframe_interval=1000)
    smooth = torch.arange(96, dtype=torch.uint8)[:, None, None].expand(96, 128, 3)
    for i in range(3):  # an IDR, then P frames at 96x128
        data = enc.encode(e(smooth.contiguous()))
        assert (H264SwCodec(EncoderConfig()).decode(data) is not None) == (i == 0)
    out = e(smooth[:48, :80].contiguous())  # the publisher drops to 48x80
    assert out.shape == (48, 80, 3)
    got = H264SwCodec(EncoderConfig()).decode(enc.encode(out))
    assert got is not None, "the first frame at a new size must be a keyframe"
    assert got.shape == (48, 80, 3)
    # and the stream goes on with P frames at the new size
    nxt = enc.encode(e(smooth[:48, :80].contiguous()))
    assert H264SwCodec(EncoderConfig()).decode(nxt) is None


def test_agent_flags_reach_the_engine_config(monkeypatch):
    """--output-size / --output-max-side travel as app keys (create_app) and
    as environment defaults (spawned workers), like --fit."""
    from ai_rtc_agent_amd.agent import create_app

    app = create_app(pool=object(), use_turn=False, output_size="source",
                     output_max_side=960)
    assert app["output_size"] == "source" and app["output_max_side"] == 960
    app = create_app(pool=object(), use_turn=False)
    assert app["output_size"] is None and app["output_max_side"] is None
    monkeypatch.setenv("AIRTC_OUTPUT_SIZE", "source")
    monkeypatch.setenv("AIRTC_OUTPUT_MAX_SIDE", "640")
    cfg = EngineConfig()
    assert (cfg.output_size, cfg.output_max_side) == ("source", 640)
