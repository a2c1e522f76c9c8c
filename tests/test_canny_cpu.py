"""Canny edge conditioning for the ControlNet path, on the CPU: the torch
form of the operator (ops.canny_hint, defined in ops/interface.py), the
engine's per-frame hint FIFO against a slow path that recomputes every
stage's hint, the per-slot threshold controls and the agent surface.

The scene and chain builders here are shared with test_canny_gpu.py.
"""
import asyncio

import pytest
import torch
from aiohttp.test_utils import TestClient, TestServer

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.agent import _apply_session_config, create_app
from ai_rtc_agent_amd.config import EngineConfig
from ai_rtc_agent_amd.engine import StreamDiffusionEngine
from ai_rtc_agent_amd.engine.scheduler import slot_rows
from ai_rtc_agent_amd.parallel.batching import BatchedPipeline
from ai_rtc_agent_amd.parallel.dispatch import PipelinePool

THR = (50, 100)
SCENE_SIZES = ((48, 80), (33, 70), (97, 131))


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def grey(img: torch.Tensor) -> torch.Tensor:
    """(H,W) float -> (H,W,3) u8 with equal channels."""
    return img.round().clamp(0, 255).to(torch.uint8).unsqueeze(-1).repeat(1, 1, 3)


def scene(H: int, W: int, seed: int = 0) -> torch.Tensor:
    """Discs of mixed contrast on a flat ground, one long faint stripe that
    runs through them, sigma = 3 noise: strong edges (the bold discs), weak
    ones that hang on them (the stripe and the faint discs) and loose weak
    ones. (H,W,3) u8, channels slightly apart so the luma weights matter."""
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32),
                            torch.arange(W, dtype=torch.float32), indexing="ij")
    img = torch.full((H, W), 90.0)
    m = min(H, W)
    # bold discs at both ends, faint ones between; all straddle the stripe
    contrasts = (110.0, 24.0, 20.0, 28.0, 90.0)
    for i, c in enumerate(contrasts):
        cy = (0.35 + 0.3 * torch.rand(1, generator=g).item()) * H
        cx = (0.1 + 0.8 * (i + 0.5) / len(contrasts)) * W
        r = (0.14 + 0.12 * torch.rand(1, generator=g).item()) * m
        img = torch.where((yy - cy) ** 2 + (xx - cx) ** 2 < r * r, img + c, img)
    # the stripe: a faint step whose upper edge is one long weak chain
    img = torch.where(yy >= H // 2, img + 26.0, img)
    img = img + 3.0 * torch.randn((H, W), generator=g)
    rgb = grey(img).to(torch.int32)
    rgb[..., 0] = (rgb[..., 0] * 15) // 16
    rgb[..., 2] = (rgb[..., 2] * 7) // 8
    return rgb.to(torch.uint8)


def chain_frame(H: int, W: int, y0: int, xb: int, length: int,
                transpose: bool = False) -> torch.Tensor:
    """One bold blob touching a straight faint line: the rows >= y0 stand
    130 above the ground at the left (the blob), fall to 30 above it over
    the 25 columns before xb and stay there for `length` columns (the line).
    The edge along row y0 is ONE horizontal chain, 1 px wide, strong where
    the blob is and weak from where the contrast has faded: the weak part
    hangs on the strong part without a gap (a blob with a hard side would
    break the chain at the T-junction). Noise-free, xb >= 25."""
    x = torch.arange(W, dtype=torch.float32)
    low = torch.where(x < xb, 90.0 + (xb - x).clamp(max=25.0) * 4.0,
                      torch.where(x < xb + length, torch.tensor(90.0),
                                  torch.tensor(60.0)))
    img = torch.full((H, W), 60.0)
    img[y0:] = low
    if transpose:
        img = img.t().contiguous()
    return grey(img)


def edges(frame: torch.Tensor, reach: int, thr=THR) -> torch.Tensor:
    """(H,W,3) u8 -> (H,W) bool through the public op (torch path on CPU)."""
    out = ops.canny_hint(frame.unsqueeze(0), thr, reach, torch.float32)
    return out[0, ..., 0] > 0


def flood(frame: torch.Tensor, thr=THR) -> torch.Tensor:
    """Unbounded hysteresis (what cv2 does): the reference run to its fixed
    point, for the length of a chain."""
    t = torch.tensor([list(thr)], dtype=torch.int32)
    return ops.canny_hint_reference(frame.unsqueeze(0), t, 10 ** 6)[0]


# ---------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------
def test_vertical_step_is_one_edge_column():
    img = torch.zeros(16, 16)
    img[:, 8:] = 255.0
    for reach in (0, 16):
        E = edges(grey(img), reach, (100, 200))
        cols = E.any(dim=0).nonzero().flatten().tolist()
        assert len(cols) == 1 and cols[0] in (7, 8), cols
        assert E[:, cols[0]].all() and int(E.sum()) == 16


def test_constant_frame_and_top_thresholds_give_nothing():
    flat = torch.full((16, 16, 3), 137, dtype=torch.uint8)
    assert not edges(flat, 16, (0, 0)).any()
    s = scene(48, 80)
    assert edges(s, 16, (0, 0)).any()
    assert not edges(s, 16, (2040, 2040)).any()


def test_channels_equal_and_values_binary():
    s = torch.stack([scene(33, 70), scene(33, 70, seed=1)])
    for dtype in (torch.float32, torch.float16):
        out = ops.canny_hint(s, THR, 8, dtype)
        assert out.shape == s.shape and out.dtype == dtype and out.is_contiguous()
        assert torch.equal(out[..., 0], out[..., 1]) and torch.equal(out[..., 0], out[..., 2])
        assert set(out.unique().tolist()) == {0.0, 1.0}
    buf = torch.full(s.shape, 7.0)
    assert ops.canny_hint(s, THR, 8, torch.float32, out=buf) is buf
    assert torch.equal(buf, ops.canny_hint(s, THR, 8, torch.float32))


@pytest.mark.parametrize("size", SCENE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reach_grows_the_edge_set_monotonically(size):
    s = scene(*size)
    E = {r: edges(s, r) for r in (0, 2, 8, 32)}
    counts = {r: int(e.sum()) for r, e in E.items()}
    frac = counts[32] / (size[0] * size[1])
    print(size, counts, f"edge fraction {frac:.3f}")
    # the scene is what it claims to be: some edges, not mostly edges
    assert 0.02 < frac < 0.2
    for a, b in ((0, 2), (2, 8), (8, 32)):
        assert not (E[a] & ~E[b]).any(), f"E({a}) is no subset of E({b})"
        assert counts[a] < counts[b], f"reach {a} -> {b} adds nothing: {counts}"
    # reach 0 is the strong set; everything kept is a candidate of the flood
    assert not (E[32] & ~flood(s)).any()


@pytest.mark.parametrize("transpose", [False, True], ids=["row", "column"])
def test_chain_keeps_exactly_reach_pixels(transpose):
    f = chain_frame(40, 100, 20, 30, 60, transpose)
    strong = edges(f, 0)
    chain = int(flood(f).sum()) - int(strong.sum())
    print("strong", int(strong.sum()), "chain length", chain)
    assert int(strong.sum()) > 0 and chain >= 60  # the 60 px line at least
    for r in (0, 4, 16):
        E = edges(f, r)
        assert not (strong & ~E).any()
        assert int(E.sum()) - int(strong.sum()) == min(r, chain), r
    # the kept pixels are the line's: consecutive along it, on the edge row
    # (the chain steps one row over where the contrast fades)
    extra = (edges(f, 16) & ~strong).nonzero()
    along, across = (0, 1) if transpose else (1, 0)
    assert set(extra[:, across].tolist()) <= {19, 20}
    a = extra[:, along].sort().values
    assert torch.equal(a, torch.arange(a[0], a[0] + 16))


def test_per_row_thresholds_equal_single_row_calls():
    s = torch.stack([scene(33, 70, seed=i) for i in range(3)])
    pairs = [(20, 60), (50, 100), (90, 400)]
    thr = torch.tensor(pairs, dtype=torch.int32)
    out = ops.canny_hint(s, thr, 8, torch.float32)
    singles = [ops.canny_hint(s[i:i + 1], pairs[i], 8, torch.float32) for i in range(3)]
    assert torch.equal(out, torch.cat(singles))
    assert len({int(o.sum()) for o in singles}) == 3  # the thresholds matter


def test_op_rejects_bad_arguments():
    s = scene(8, 8).unsqueeze(0)
    for thr in ((-1, 5), (10, 5), (0, 2041), (1.5, 3), (True, 3), (1, 2, 3)):
        with pytest.raises(ValueError):
            ops.canny_hint(s, thr, 4, torch.float32)
    for reach in (-1, 33, 2.0, True):
        with pytest.raises(ValueError):
            ops.canny_hint(s, THR, reach, torch.float32)
    with pytest.raises(ValueError):
        ops.canny_hint(s[0], THR, 4, torch.float32)  # (H,W,3)
    with pytest.raises(ValueError):
        ops.canny_hint(s, torch.tensor([[1, 2], [3, 4]], dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        ops.canny_hint(s, torch.tensor([[1, 2]], dtype=torch.int64), 4)
    with pytest.raises(TypeError):
        ops.canny_hint(s.float(), THR, 4)
    with pytest.raises(TypeError):
        ops.canny_hint(s, THR, 4, torch.bfloat16)
    with pytest.raises(ValueError):
        ops.canny_hint(s, THR, 4, torch.float32, out=torch.zeros(1, 8, 8, 3, dtype=torch.float16))


# ---------------------------------------------------------------------------
# engine: FIFO, encode-once, controls
# ---------------------------------------------------------------------------
def unzero(eng, seed=5):
    """Seeded non-zero weights in the ControlNet's zero-convs (stand-in for
    trained ones): without them the hint cannot reach the output."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for zc in list(eng.controlnet.zero_convs) + [eng.controlnet.mid_zero]:
            w = torch.randn(zc.weight.shape, generator=g) * 0.2
            zc.weight.copy_(w.to(zc.weight))
    return eng


def make_engine(cfg, **kw):
    args = dict(use_controlnet=True, controlnet_processor="canny",
                canny_low=THR[0], canny_high=THR[1], canny_reach=8)
    args.update(kw)
    for k, v in args.items():
        setattr(cfg, k, v)
    cfg.__post_init__()
    eng = unzero(StreamDiffusionEngine(cfg))
    eng.prepare()
    return eng


def engine_frames(n, fbs, size=64):
    return [torch.stack([scene(size, size, seed=10 * t + s) for s in range(fbs)])
            for t in range(n)]


class ChunkedEncoder(torch.nn.Module):
    """A hint encoder applied `rows` batch rows at a time. The engine
    encodes the fbs rows of a frame in one call; f32 convolutions on the
    CPU sum in an order that depends on the batch size (seen: one u8 level
    at a few pixels of the output), so the slow path encodes its B rows in
    the same portions and the comparison is exact."""

    def __init__(self, enc, rows):
        super().__init__()
        self.enc, self.rows = enc, rows

    def forward(self, hint):
        return torch.cat([self.enc(hint[i:i + self.rows])
                          for i in range(0, hint.shape[0], self.rows)])


class SlowControl:
    """The ControlNet call of an engine, replaced by the slow path: every
    row's hint is recomputed at full resolution from the frame its stage is
    working on (test-side history) and goes through ControlNet(hint=...).
    The features the engine hands in are ignored."""

    def __init__(self, eng):
        self.eng, self.cn = eng, eng.controlnet
        self.cn.hint_encoder = ChunkedEncoder(self.cn.hint_encoder,
                                              eng.cfg.frame_buffer_size)
        self.cfg, self.hint_encoder = self.cn.cfg, self.cn.hint_encoder
        self.history = []  # newest first, (fbs,H,W,3) u8 each

    def __call__(self, sample, ts, emb, scale=1.0, hint_features=None):
        cfg = self.eng.cfg
        fbs, n = cfg.frame_buffer_size, cfg.denoising_steps
        self.history.insert(0, self.eng._frame_in.clone())
        rows = [self.history[i] if i < len(self.history)
                else torch.zeros_like(self.history[0]) for i in range(n)]
        thr = self.eng._canny_thr
        hint = torch.cat([ops.canny_hint(r, thr, cfg.canny_reach, self.eng.dtype)
                          for r in rows])
        layout = self.eng._layout()
        if layout == "full":
            hint = torch.cat([hint, hint])
        elif layout == "initialize":
            hint = torch.cat([hint[:fbs], hint])
        assert hint.shape[0] == sample.shape[0]
        return self.cn(sample, ts, emb, hint, scale=scale)


@pytest.mark.parametrize("variant", ["fbs1", "fbs2", "fbs2_full"])
def test_fifo_holds_each_stage_its_own_frame(tiny_cfg, variant):
    import copy

    kw = {"fbs1": dict(frame_buffer_size=1),
          "fbs2": dict(frame_buffer_size=2),
          "fbs2_full": dict(frame_buffer_size=2, cfg_type="full", guidance_scale=1.4,
                            negative_prompt="blurry")}[variant]
    fbs = kw["frame_buffer_size"]
    eng = make_engine(copy.deepcopy(tiny_cfg), **kw)
    slow = make_engine(copy.deepcopy(tiny_cfg), **kw)
    slow.controlnet = SlowControl(slow)
    n = eng.cfg.denoising_steps
    assert n == 4 and eng._hint_feat_buffer.shape[0] == (n - 1) * fbs
    assert (eng._layout() == "full") == (variant == "fbs2_full")
    assert not eng._hint_feat_buffer.any()

    frames = engine_frames(6, fbs)
    feats = []  # newest first: hint_encoder(canny_hint(frame)) per call
    differ = 0
    for t, f in enumerate(frames):
        out = eng(f).clone()
        want = slow(f).clone()
        with torch.no_grad():
            feats.insert(0, eng.controlnet.hint_encoder(
                ops.canny_hint(f, THR, 8, torch.float32)))
        buf = eng._hint_feat_buffer
        for j in range(n - 1):  # block j: what stage j+1 reads next call
            got = buf[j * fbs:(j + 1) * fbs]
            if j <= t:
                assert torch.equal(got, feats[j]), (t, j)
            else:
                assert not got.any(), (t, j)
        if t >= n - 1:
            # every stage of this output's history saw a real frame
            assert torch.equal(out, want), f"frame {t}"
        if t > 0:
            differ += int(not torch.equal(out, prev))
        prev = out
    assert differ > 0, "the outputs never move: the test would pass on anything"


def test_hint_reaches_the_output_and_none_is_the_old_path(tiny_cfg):
    import copy

    base = dict(use_controlnet=True)
    frames = engine_frames(5, 1)

    def run(**kw):
        cfg = copy.deepcopy(tiny_cfg)
        for k, v in {**base, **kw}.items():
            setattr(cfg, k, v)
        eng = unzero(StreamDiffusionEngine(cfg))
        eng.prepare()
        return eng, torch.stack([eng(f).clone() for f in frames])

    old_eng, old = run()
    none_eng, none = run(controlnet_processor="none", canny_low=7, canny_high=9,
                         canny_reach=3)
    assert torch.equal(old, none)
    assert none_eng._hint_feat_buffer is None and none_eng._canny_thr is None
    assert "controlnet" not in none_eng.stats()
    assert "canny_low" not in none_eng.slot_controls(0)
    with pytest.raises(ValueError):
        none_eng.update_canny(10, 20)
    _, canny = run(controlnet_processor="canny", canny_low=50, canny_high=100)
    _, loose = run(controlnet_processor="canny", canny_low=5, canny_high=10)
    assert not torch.equal(canny, old)
    assert not torch.equal(canny, loose)  # the thresholds reach the frames


def test_controlnet_forward_takes_features_or_hint():
    from ai_rtc_agent_amd.models import UNetConfig
    from ai_rtc_agent_amd.models.controlnet import ControlNet

    torch.manual_seed(0)
    cn = ControlNet(UNetConfig.tiny()).eval()
    for zc in list(cn.zero_convs) + [cn.mid_zero]:
        torch.nn.init.normal_(zc.weight, std=0.1)
    x, t = torch.randn(2, 8, 8, 4), torch.tensor([100, 300])
    ctx = torch.randn(2, 77, cn.cfg.cross_attention_dim)
    hint = torch.rand(2, 64, 64, 3)
    with torch.no_grad():
        a = cn(x, t, ctx, hint, 0.5)
        b = cn(x, t, ctx, scale=0.5, hint_features=cn.hint_encoder(hint))
        for u, v in zip(a[0] + [a[1]], b[0] + [b[1]]):
            assert torch.equal(u, v)
        with pytest.raises(ValueError):
            cn(x, t, ctx)
        with pytest.raises(ValueError):
            cn(x, t, ctx, hint, hint_features=cn.hint_encoder(hint))


def test_config_validation():
    for kw in (dict(controlnet_processor="hed"), dict(canny_low=-1),
               dict(canny_low=300, canny_high=200), dict(canny_high=2041),
               dict(canny_reach=33), dict(canny_reach=-1), dict(canny_low=1.5),
               dict(canny_reach=True)):
        with pytest.raises(ValueError):
            EngineConfig(**kw)
    c = EngineConfig()
    assert (c.controlnet_processor, c.canny_low, c.canny_high, c.canny_reach) == \
        ("none", 100, 200, 16)


def test_config_reads_the_environment(monkeypatch):
    monkeypatch.setenv("AIRTC_CONTROLNET_PROCESSOR", "canny")
    monkeypatch.setenv("AIRTC_CANNY_LOW", "30")
    monkeypatch.setenv("AIRTC_CANNY_HIGH", "90")
    monkeypatch.setenv("AIRTC_CANNY_REACH", "4")
    c = EngineConfig()
    assert (c.controlnet_processor, c.canny_low, c.canny_high, c.canny_reach) == \
        ("canny", 30, 90, 4)
    monkeypatch.setenv("AIRTC_CANNY_REACH", "40")
    with pytest.raises(ValueError):
        EngineConfig()


def test_update_canny_is_per_slot_and_reset_restores(tiny_cfg):
    import copy

    kw = dict(frame_buffer_size=2)
    eng = make_engine(copy.deepcopy(tiny_cfg), **kw)
    ref = make_engine(copy.deepcopy(tiny_cfg), **kw)
    frames = engine_frames(9, 2)
    for f in frames[:4]:
        assert torch.equal(eng(f), ref(f))
    thr_ptr = eng._canny_thr.data_ptr()
    eng.update_canny(5, 12, slot=1)
    assert eng._canny_thr.tolist() == [[50, 100], [5, 12]]
    assert eng._canny_thr.data_ptr() == thr_ptr  # written in place
    assert eng.slot_controls(1)["canny_low"] == 5 and eng.slot_controls(0)["canny_low"] == 50
    assert eng.stats()["controlnet"] == {
        "processor": "canny", "scale": 1.0, "canny_reach": 8,
        "canny_thresholds": [[50, 100], [5, 12]]}
    # a frame is conditioned on its own hint through all four stages: the
    # three in flight keep the hints they were encoded with, so the first
    # frame encoded under the new thresholds comes out three calls later
    for i, f in enumerate(frames[4:8]):
        a, b = eng(f), ref(f)
        assert torch.equal(a[0], b[0]), "slot 0 noticed slot 1's thresholds"
        assert torch.equal(a[1], b[1]) == (i < 3), i
    eng.update_canny(high=300, slot=1)  # one value: the other stays
    assert eng._canny_thr.tolist() == [[50, 100], [5, 300]]

    for bad in ((-1, 5), (10, 5), (0, 2041), (1.5, 3), ("a", 3)):
        with pytest.raises(ValueError):
            eng.update_canny(*bad, slot=0)
    with pytest.raises(ValueError):
        eng.update_canny(400, slot=1)  # above the slot's own high
    with pytest.raises(ValueError):
        eng.update_canny(10, 20, slot=2)
    assert eng._canny_thr.tolist() == [[50, 100], [5, 300]]

    # reset: FIFO rows of the slot zeroed, thresholds back, slot 0 untouched
    before = eng._hint_feat_buffer.clone()
    assert slot_rows(before, 1, 2).any()
    eng.reset_slot(1)
    assert not slot_rows(eng._hint_feat_buffer, 1, 2).any()
    assert torch.equal(slot_rows(eng._hint_feat_buffer, 0, 2), slot_rows(before, 0, 2))
    assert eng._canny_thr.tolist() == [[50, 100], [50, 100]]
    assert eng.slot_controls(1) == ref.slot_controls(1)
    # the reset slot now equals a freshly prepared engine's first frame
    fresh = make_engine(copy.deepcopy(tiny_cfg), **kw)
    assert torch.equal(eng(frames[8])[1], fresh(frames[8])[1])

    # replica-wide: every slot and the defaults a reset restores
    eng.update_canny(20, 40)
    assert eng._canny_thr.tolist() == [[20, 40], [20, 40]]
    assert (eng.cfg.canny_low, eng.cfg.canny_high) == (20, 40)
    eng.update_canny(30, 60, slot=0)
    eng.reset_slot(0)
    assert eng._canny_thr.tolist() == [[20, 40], [20, 40]]


def test_reprepare_keeps_a_slots_thresholds(tiny_cfg):
    import copy

    eng = make_engine(copy.deepcopy(tiny_cfg), frame_buffer_size=2)
    eng.update_canny(7, 9, slot=1)
    eng.update_t_index_list([10, 30])  # another length: prepare() again
    assert eng._hint_feat_buffer.shape[0] == 2
    assert eng._canny_thr.tolist() == [[50, 100], [7, 9]]
    assert eng.slot_controls(1)["canny_high"] == 9


def test_one_step_engine_has_an_empty_fifo(tiny_cfg):
    import copy

    eng = make_engine(copy.deepcopy(tiny_cfg), t_index_list=[20])
    assert eng._hint_feat_buffer.shape[0] == 0
    f = engine_frames(1, 1)[0]
    assert eng(f).shape == (1, 64, 64, 3)
    eng.reset_slot(0)


# ---------------------------------------------------------------------------
# agent surface
# ---------------------------------------------------------------------------
def run_async(coro, timeout=60):
    loop = asyncio.new_event_loop()
    try:
        return loop.run_until_complete(asyncio.wait_for(coro, timeout))
    finally:
        loop.close()


OFFER_SDP = "\r\n".join([
    "v=0", "o=- 1 2 IN IP4 127.0.0.1", "s=-", "t=0 0",
    "m=video 51000 UDP/TLS/RTP/SAVPF 97",
    "a=ice-ufrag:abcd", "a=ice-pwd:efghijklmnop", "a=mid:0", "a=sendrecv",
    "a=rtpmap:97 H264/90000",
    "a=candidate:1 1 udp 2130706431 127.0.0.1 51000 typ host",
]) + "\r\n"


class Pipe:
    """StreamDiffusionPipeline's surface over a tiny engine."""

    def __init__(self, eng):
        self.engine, self.cfg = eng, eng.cfg
        for name in ("update_prompt", "update_canny", "reset_slot",
                     "slot_controls", "stats"):
            setattr(self, name, getattr(eng, name))

    def __call__(self, frames):
        return self.engine(frames)


def test_agent_config_and_stats(tiny_cfg):
    import copy

    eng = make_engine(copy.deepcopy(tiny_cfg), frame_buffer_size=2)

    async def body():
        pool = PipelinePool([BatchedPipeline(Pipe(eng), 2)])
        client = TestClient(TestServer(create_app(pool=pool, use_turn=False)))
        await client.start_server()
        sids = []
        for _ in range(2):
            r = await client.post("/whip", data=OFFER_SDP,
                                  headers={"Content-Type": "application/sdp"})
            assert r.status == 201
            sids.append(r.headers["Location"].rsplit("/", 1)[1])

        r = await client.post("/config", json={
            "stream_id": sids[1], "canny_low": 11, "canny_high": 22})
        assert r.status == 200
        assert eng._canny_thr.tolist() == [[50, 100], [11, 22]]
        r = await client.post("/config", json={"stream_id": sids[0], "canny_high": 500})
        assert r.status == 200
        assert eng._canny_thr.tolist() == [[50, 500], [11, 22]]

        for bad in ({"canny_low": "5"}, {"canny_low": True}, {"canny_high": 2041},
                    {"canny_low": -1}, {"canny_low": 1.5},
                    {"canny_low": 30, "canny_high": 20},
                    {"stream_id": sids[1], "canny_low": 30}):  # above its high
            r = await client.post("/config", json=bad)
            assert r.status == 400, bad
        assert eng._canny_thr.tolist() == [[50, 500], [11, 22]]
        r = await client.post("/config", json={"stream_id": "nope", "canny_low": 1})
        assert r.status == 404

        r = await client.get("/stats")
        rep = (await r.json())["per_replica"][0]
        assert rep["controlnet"] == {
            "processor": "canny", "scale": 1.0, "canny_reach": 8,
            "canny_thresholds": [[50, 500], [11, 22]]}
        assert rep["per_stream"][1]["canny_low"] == 11

        r = await client.post("/config", json={"canny_low": 40, "canny_high": 80})
        assert r.status == 200  # no stream_id: every slot
        assert eng._canny_thr.tolist() == [[40, 80], [40, 80]]
        await client.close()

    run_async(body())


def test_datachannel_canny_is_per_session(tiny_cfg):
    import copy

    eng = make_engine(copy.deepcopy(tiny_cfg), frame_buffer_size=2)
    bp = BatchedPipeline(Pipe(eng), 2)

    async def body():
        a, b = bp.acquire("a"), bp.acquire("b")
        _apply_session_config(b, {"canny_low": 3, "canny_high": 4})
        _apply_session_config(a, {"canny_low": "x"})   # logged, ignored
        _apply_session_config(a, {"canny_low": 1000})  # above a's high: ignored
        assert eng._canny_thr.tolist() == [[50, 100], [3, 4]]
        bp.release("b")
        bp.acquire("c")  # slot 1 again, handed out reset
        assert eng._canny_thr.tolist() == [[50, 100], [50, 100]]
        bp.release("a")
        bp.release("c")

    run_async(body())


def test_agent_flags_switch_the_controlnet_on(monkeypatch):
    """--controlnet-processor canny implies use_controlnet; the flags reach
    the EngineConfig the pool is built with."""
    import ai_rtc_agent_amd.parallel.dispatch as dispatch

    seen = {}

    def fake_create(model_id, n_gpus, cfg, streams_per_replica=1):
        seen["cfg"] = cfg
        return PipelinePool([])

    monkeypatch.setattr(dispatch.PipelinePool, "create", staticmethod(fake_create))

    async def body(**kw):
        app = create_app(use_turn=False, **kw)
        client = TestClient(TestServer(app))
        await client.start_server()
        await client.close()
        return seen.pop("cfg")

    cfg = run_async(body(controlnet_processor="canny", controlnet_scale=0.7,
                         canny_low=30, canny_high=90, canny_reach=4))
    assert cfg.use_controlnet and cfg.controlnet_processor == "canny"
    assert (cfg.controlnet_scale, cfg.canny_low, cfg.canny_high, cfg.canny_reach) == \
        (0.7, 30, 90, 4)
    cfg = run_async(body())
    assert not cfg.use_controlnet and cfg.controlnet_processor == "none"
    with pytest.raises(Exception):
        run_async(body(controlnet_processor="canny", canny_low=300, canny_high=100))
