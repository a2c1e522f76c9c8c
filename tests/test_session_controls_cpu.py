"""Per-session prompt, guidance and strength under batched serving — CPU.

K sessions share one engine whose batch dimension is the K streams; these
tests pin that each session's controls reach its own rows only:

- ops.rcfg_apply (the per-row RCFG step; here its torch fallback) against
  the scalar chain of ResidualCFG,
- the engine "triangle": a run with per-slot controls (A, B) equals, slot by
  slot and bit for bit, the runs with (A, A) and (B, B) — rows are
  independent and the shapes identical, so anything but exact equality would
  mean some op mixes batch rows,
- reset_slot, runtime_guidance, and the serving/API plumbing with stubs.
"""
import asyncio
import functools

import pytest
import torch
from aiohttp.test_utils import TestClient, TestServer

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.agent import _apply_session_config, create_app
from ai_rtc_agent_amd.config import EngineConfig
from ai_rtc_agent_amd.engine import StreamDiffusionEngine
from ai_rtc_agent_amd.engine.rcfg import ResidualCFG
from ai_rtc_agent_amd.engine.scheduler import slot_rows
from ai_rtc_agent_amd.parallel.batching import BatchedPipeline
from ai_rtc_agent_amd.parallel.dispatch import PipelinePool

B, FBS = 6, 2
MODES = ("self", "initialize", "full")
# per_b = 64, 24 (8 * odd) and 12 (no multiple of 8: the scalar path)
SHAPES = ((B, 4, 4, 4), (B, 1, 6, 4), (B, 1, 3, 4))
G_ROWS = (1.5, 3.0, 0.5, 2.25, 1.0, 7.5)
D_ROWS = (1.0, 0.5, 0.7, 1.0, 0.9, 0.3)


def rcfg_inputs(mode, shape, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    rows = {"self": B, "initialize": B + FBS, "full": 2 * B}[mode]
    eps = torch.randn((rows, *shape[1:]), generator=gen).to(dtype)
    stock = torch.randn(shape, generator=gen).to(dtype)
    return eps, stock


def scalar_chain(mode, eps, stock, g, delta):
    """ResidualCFG's scalar path (no reset(): no per-row tensors) on clones.
    Returns (out, stock after). At g <= 1 the chain still runs, with the
    effective scale 1 (runtime=True), as a g <= 1 row of a batch does."""
    r = ResidualCFG(mode, g, delta, runtime=g <= 1.0)
    r.stock_noise = stock.clone()
    assert r.gm1_rows is None
    out = r.apply(eps.clone(), FBS)
    return out, r.stock_noise


def coef(vals):
    return torch.tensor(vals, dtype=torch.float32)


def apply_rows(mode, eps, stock, g_rows, d_rows):
    g_eff = [max(g, 1.0) for g in g_rows]
    stock = stock.clone()
    if mode == "full":
        return ops.rcfg_apply("full", eps.clone(), FBS, g=coef(g_eff)), stock
    out = ops.rcfg_apply(
        mode, eps.clone(), FBS, stock=stock, delta=coef(d_rows),
        gm1=torch.tensor([g - 1.0 for g in g_eff], dtype=torch.float64).float())
    return out, stock


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_rcfg_apply_uniform_equals_scalar_chain(mode, shape, dtype):
    eps, stock = rcfg_inputs(mode, shape, dtype)
    want, want_stock = scalar_chain(mode, eps, stock, 1.5, 0.7)
    got, got_stock = apply_rows(mode, eps, stock, [1.5] * B, [0.7] * B)
    assert got.shape == shape and got.dtype == dtype
    assert torch.equal(got, want)
    if mode != "full":
        assert torch.equal(got_stock, want_stock)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_rcfg_apply_per_row_equals_scalar_chain_per_row(mode, shape, dtype):
    eps, stock = rcfg_inputs(mode, shape, dtype, seed=1)
    got, got_stock = apply_rows(mode, eps, stock, G_ROWS, D_ROWS)
    eps_c = eps[eps.shape[0] - B:]
    for r in range(B):
        want, want_stock = scalar_chain(mode, eps, stock, G_ROWS[r], D_ROWS[r])
        assert torch.equal(got[r], want[r]), f"row {r}"
        if mode != "full":
            # the shift does not depend on the coefficients
            assert torch.equal(got_stock, want_stock)
        if mode != "full" and G_ROWS[r] <= 1.0:
            # per-row "inactive": eps passes through bit-exactly
            assert torch.equal(got[r], eps_c[r]), f"row {r}"


def test_rcfg_apply_rejects_bad_arguments():
    eps, stock = rcfg_inputs("self", SHAPES[0], torch.float32)
    with pytest.raises(ValueError):
        ops.rcfg_apply("bogus", eps, FBS, gm1=coef([0.5] * B),
                       delta=coef([1.0] * B), stock=stock)
    with pytest.raises(ValueError):
        ops.rcfg_apply("self", eps, FBS, gm1=coef([0.5] * B))


def test_slot_rows_is_the_row_law():
    t = torch.arange(12).view(6, 2)
    assert slot_rows(t, None, 2) is t
    assert slot_rows(t, 1, 2)[:, 0].tolist() == [2, 6, 10]  # rows 1, 3, 5
    slot_rows(t, 0, 2).zero_()  # a view: writes land in t
    assert t[::2].sum() == 0 and t[1::2].sum() > 0
    with pytest.raises(ValueError):
        slot_rows(t, 2, 2)
    with pytest.raises(ValueError):
        slot_rows(t, 0, 4)


def test_residual_cfg_set_guidance_rows():
    r = ResidualCFG("self", 1.5, 0.7)
    r.reset(torch.zeros(B, 2, 2, 4))
    assert r.gm1_rows.tolist() == [0.5] * B
    r.set_guidance(guidance_scale=3.0, slot=1, fbs=FBS)
    r.set_guidance(delta=0.25, slot=0, fbs=FBS)
    assert r.gm1_rows.tolist() == [0.5, 2.0] * 3
    assert r.delta_rows.tolist() == [0.25, coef([0.7]).item()] * 3
    assert r.guidance_scale == 1.5  # a slot write leaves the scalars alone
    r.set_guidance(guidance_scale=0.0, slot=0, fbs=FBS)  # max(g, 1) - 1 = 0
    assert r.gm1_rows.tolist() == [0.0, 2.0] * 3 and r.active
    r.set_guidance(guidance_scale=2.0, delta=1.0)
    assert r.gm1_rows.tolist() == [1.0] * B and r.guidance_scale == 2.0
    assert r.delta_rows.tolist() == [1.0] * B and r.delta == 1.0


# ---------------------------------------------------------------------------
# engine: model_family tiny, 64x64, fbs=2, two stages
# ---------------------------------------------------------------------------
PROMPT_A = "a watercolour painting of a harbour at dawn"
PROMPT_B = "neon cyberpunk alley in heavy rain"
N_FRAMES = 4


def make_engine(**kw):
    args = dict(model_family="tiny", width=64, height=64, device="cpu",
                acceleration="eager", use_hip_graph=False, use_lcm_lora=False,
                t_index_list=[10, 30], cfg_type="self", guidance_scale=1.5,
                frame_buffer_size=FBS)
    args.update(kw)
    eng = StreamDiffusionEngine(EngineConfig(**args))
    eng.prepare()
    return eng


@functools.lru_cache(maxsize=None)
def frames(n=N_FRAMES):
    gen = torch.Generator().manual_seed(7)
    return torch.randint(0, 256, (n, FBS, 64, 64, 3), generator=gen,
                         dtype=torch.uint8)


def run_frames(eng, lo=0, hi=N_FRAMES):
    """(hi - lo, FBS, 64, 64, 3) outputs; frames differ per slot."""
    return torch.stack([eng(frames(max(hi, N_FRAMES))[i]).clone()
                        for i in range(lo, hi)])


def triangle(setup, a, b, **kw):
    """Outputs of the runs with per-slot controls (a, b), (a, a), (b, b)."""
    outs = []
    for s0, s1 in ((a, b), (a, a), (b, b)):
        eng = make_engine(**kw)
        setup(eng, s0, 0)
        setup(eng, s1, 1)
        outs.append(run_frames(eng))
    return outs


def assert_triangle(x, y, z):
    assert not torch.equal(y[:, 0], z[:, 0]), "the control changes nothing"
    assert not torch.equal(y[:, 1], z[:, 1]), "the control changes nothing"
    assert torch.equal(x[:, 0], y[:, 0])
    assert torch.equal(x[:, 1], z[:, 1])


def test_engine_per_slot_prompt():
    x, y, z = triangle(lambda e, v, s: e.update_prompt(v, slot=s),
                       PROMPT_A, PROMPT_B)
    assert_triangle(x, y, z)


def test_engine_per_slot_guidance():
    x, y, z = triangle(lambda e, v, s: e.update_guidance(v, slot=s), 1.0, 2.0)
    assert_triangle(x, y, z)


def test_engine_per_slot_delta():
    x, y, z = triangle(lambda e, v, s: e.update_guidance(delta=v, slot=s),
                       1.0, 0.5)
    assert_triangle(x, y, z)


def test_engine_per_slot_t_index_list():
    x, y, z = triangle(lambda e, v, s: e.update_t_index_list(v, slot=s),
                       [10, 30], [5, 45])
    assert_triangle(x, y, z)


def test_engine_per_slot_negative_prompt_cfg_full():
    x, y, z = triangle(lambda e, v, s: e.update_negative_prompt(v, slot=s),
                       PROMPT_A, PROMPT_B, cfg_type="full")
    assert_triangle(x, y, z)


def test_engine_per_slot_prompt_cfg_full_and_initialize():
    for cfg_type in ("full", "initialize"):
        x, y, z = triangle(lambda e, v, s: e.update_prompt(v, slot=s),
                           PROMPT_A, PROMPT_B, cfg_type=cfg_type)
        assert_triangle(x, y, z)


def test_engine_per_slot_guidance_cfg_full_and_initialize():
    for cfg_type in ("full", "initialize"):
        x, y, z = triangle(lambda e, v, s: e.update_guidance(v, slot=s),
                           1.25, 2.0, cfg_type=cfg_type)
        assert_triangle(x, y, z)


def test_engine_per_slot_prompt_sdxl_added_cond():
    x, y, z = triangle(lambda e, v, s: e.update_prompt(v, slot=s),
                       PROMPT_A, PROMPT_B, model_family="tiny_xl")
    assert_triangle(x, y, z)


def test_global_updates_keep_their_meaning():
    """slot=None is every slot: a global update equals the same update made
    slot by slot wherever both take the same arithmetic path (guidance,
    t_index_list), and it moves the defaults."""
    a, b = make_engine(), make_engine()
    a.update_guidance(2.0, 0.5)
    a.update_t_index_list([5, 45])
    for s in range(FBS):
        b.update_guidance(2.0, 0.5, slot=s)
        b.update_t_index_list([5, 45], slot=s)
    assert torch.equal(run_frames(a), run_frames(b))
    assert a.cfg.guidance_scale == 2.0 and a.cfg.t_index_list == [5, 45]
    assert b.cfg.guidance_scale == 1.5 and b.cfg.t_index_list == [10, 30]
    assert a.slot_controls(0) == b.slot_controls(0)


def test_per_slot_t_index_list_must_keep_length():
    eng = make_engine()
    with pytest.raises(ValueError):
        eng.update_t_index_list([10], slot=0)
    with pytest.raises(ValueError):
        eng.update_t_index_list([10, 99], slot=0)  # outside the timetable
    with pytest.raises(ValueError):
        eng.update_prompt("x", slot=FBS)
    assert eng.slot_controls(0)["t_index_list"] == [10, 30]


def test_slot_controls_and_negative_prompt_store():
    eng = make_engine()  # cfg self: the negative prompt is only stored
    before = run_frames(eng, 0, 1)
    eng.update_negative_prompt("blurry", slot=1)
    eng.update_prompt(PROMPT_B, slot=1)
    eng.update_guidance(2.0, slot=1)
    assert eng.slot_controls(0) == {
        "prompt": eng.cfg.prompt, "negative_prompt": "", "guidance_scale": 1.5,
        "delta": 1.0, "t_index_list": [10, 30]}
    assert eng.slot_controls(1) == {
        "prompt": PROMPT_B, "negative_prompt": "blurry", "guidance_scale": 2.0,
        "delta": 1.0, "t_index_list": [10, 30]}
    assert before.shape == (1, FBS, 64, 64, 3)


def test_reset_slot_restores_state_and_controls():
    """3 frames, reset slot 1, 3 more: slot 1 continues as a fresh engine's
    slot 1 would, slot 0 as if nothing had happened."""
    eng = make_engine()
    eng.update_guidance(3.0, 0.5, slot=1)      # the first tenant's controls
    eng.update_t_index_list([5, 45], slot=1)
    first = run_frames(eng, 0, 3)
    eng.reset_slot(1)
    assert eng.slot_controls(1) == eng.slot_controls(0)
    assert eng.stats()["ingest"]["last_source_size"][1] is None
    second = run_frames(eng, 3, 6)

    fresh = run_frames(make_engine(), 3, 6)
    assert torch.equal(second[:, 1], fresh[:, 1])
    never = make_engine()
    never_out = run_frames(never, 0, 6)
    assert torch.equal(first[:, 0], never_out[:3, 0])
    assert torch.equal(second[:, 0], never_out[3:, 0])
    # without the reset the previous tenant's latents would show
    assert not torch.equal(never_out[3:, 1], fresh[:, 1])


def test_reset_slot_restores_prompt():
    eng = make_engine()
    eng.update_prompt(PROMPT_B, slot=1)
    run_frames(eng, 0, 2)
    eng.reset_slot(1)
    assert eng.slot_controls(1)["prompt"] == eng.cfg.prompt
    # against an engine whose slot 1 was given the default prompt the same
    # way (one-row K|V projection)
    ref = make_engine()
    ref.update_prompt(ref.cfg.prompt, slot=1)
    assert torch.equal(run_frames(eng, 2, 4)[:, 1], run_frames(ref, 2, 4)[:, 1])


def test_runtime_guidance_flag():
    off = make_engine(guidance_scale=0.0)
    on = make_engine(guidance_scale=0.0, runtime_guidance=True)
    assert not off.rcfg.active and on.rcfg.active
    base = run_frames(off)
    assert torch.equal(run_frames(on), base)
    # a later per-slot raise changes that slot alone
    on2 = make_engine(guidance_scale=0.0, runtime_guidance=True)
    on2.update_guidance(2.0, slot=1)
    out = run_frames(on2)
    assert torch.equal(out[:, 0], base[:, 0])
    assert not torch.equal(out[:, 1], base[:, 1])


def test_per_slot_raise_without_the_flag_is_an_error():
    eng = make_engine(guidance_scale=0.0)
    with pytest.raises(ValueError, match="runtime_guidance"):
        eng.update_guidance(2.0, slot=1)
    eng.update_guidance(0.5, slot=1)  # nothing to raise: stored
    assert eng.slot_controls(1)["guidance_scale"] == 0.5
    with pytest.raises(ValueError):
        eng.update_guidance("strong", slot=1)


def test_global_raise_on_inactive_engine_reprepares():
    eng = make_engine(guidance_scale=0.0)
    eng.update_guidance(1.5)
    assert eng.rcfg.active and eng.cfg.guidance_scale == 1.5
    assert torch.equal(run_frames(eng), run_frames(make_engine()))


def test_reprepare_keeps_the_sessions_own_controls():
    """A replica-wide guidance raise on an inactive engine re-prepares; what
    a slot had moved away from the defaults is written again afterwards."""
    eng = make_engine(guidance_scale=0.0)
    eng.update_prompt(PROMPT_B, slot=1)
    eng.update_t_index_list([5, 45], slot=1)
    eng.update_guidance(delta=0.5, slot=0)
    run_frames(eng, 0, 1)
    eng.update_guidance(1.5)  # re-prepare: RCFG enters the step
    assert eng.rcfg.active
    assert eng.slot_controls(1) == {
        "prompt": PROMPT_B, "negative_prompt": "", "guidance_scale": 1.5,
        "delta": 1.0, "t_index_list": [5, 45]}
    assert eng.slot_controls(0)["delta"] == 0.5
    assert eng.slot_controls(0)["prompt"] == eng.cfg.prompt
    ref = make_engine(guidance_scale=1.5)
    ref.update_prompt(PROMPT_B, slot=1)
    ref.update_t_index_list([5, 45], slot=1)
    ref.update_guidance(delta=0.5, slot=0)
    assert torch.equal(run_frames(eng), run_frames(ref))

    # another length: the prompt stays, the old-length list cannot
    eng.update_t_index_list([10, 20, 30])
    c = eng.slot_controls(1)
    assert c["prompt"] == PROMPT_B and c["t_index_list"] == [10, 20, 30]
    assert eng.slot_controls(0)["delta"] == 0.5
    assert run_frames(eng, 0, 1).shape == (1, FBS, 64, 64, 3)


def test_reset_slot_forbids_a_filter_skip_of_the_next_call():
    """A similarity-filter skip returns the previous output, which holds the
    previous tenant's frame: the call after a reset must run."""
    from ai_rtc_agent_amd.config import SimilarityFilterConfig

    eng = make_engine(similarity_filter=SimilarityFilterConfig(
        enabled=True, threshold=0.0, max_skip_frame=1000))
    f = frames()[0]
    first = eng(f).clone()
    assert eng._prev_out is not None
    eng.reset_slot(1)
    assert eng._prev_out is None
    calls = []
    real = eng._step_core
    eng._step_core = lambda: (calls.append(1), real())[1]
    eng(f)
    assert calls == [1] and first.shape == (FBS, 64, 64, 3)


def test_uniform_rows_without_a_kernel_take_the_scalar_chain(monkeypatch):
    """CPU / forced eager with every row at the scalars: ResidualCFG runs
    the chain it always ran; ops.rcfg_apply's torch fallback is for rows
    that differ."""
    import ai_rtc_agent_amd.engine.rcfg as rcfg_mod

    calls = []
    real = rcfg_mod.ops.rcfg_apply
    monkeypatch.setattr(rcfg_mod.ops, "rcfg_apply",
                        lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    r = ResidualCFG("self", 1.5, 0.7)
    r.reset(torch.zeros(B, 2, 2, 4))
    eps = torch.randn(B, 2, 2, 4)
    r.apply(eps, FBS)
    assert calls == []
    r.set_guidance(2.0, slot=1, fbs=FBS)
    r.apply(eps, FBS)
    assert calls == ["self"]
    r.set_guidance(2.0, 0.7)  # replica-wide, both values: uniform again
    r.apply(eps, FBS)
    assert calls == ["self"]


# ---------------------------------------------------------------------------
# serving + API, with recording stubs
# ---------------------------------------------------------------------------
class RecordingPipeline:
    """Pipeline stub with the slot-addressed update surface."""

    def __init__(self, slots=2, h=8, w=8):
        self.cfg = EngineConfig(width=w, height=h)
        self.cfg.frame_buffer_size = slots
        self.slots = slots
        self.log = []

    def __call__(self, batch):
        return batch

    def update_prompt(self, prompt, slot=None):
        self.log.append(("prompt", prompt, slot))

    def update_negative_prompt(self, prompt, slot=None):
        self.log.append(("negative_prompt", prompt, slot))

    def update_guidance(self, guidance_scale=None, delta=None, slot=None):
        self.log.append(("guidance", guidance_scale, delta, slot))

    def update_t_index_list(self, t, slot=None):
        if slot is not None and len(t) != 2:
            raise ValueError("a per-slot t_index_list must keep the length")
        self.log.append(("t_index_list", list(t), slot))

    def reset_slot(self, slot):
        self.log.append(("reset", slot))

    def slot_controls(self, slot):
        return {"prompt": f"p{slot}", "negative_prompt": "", "guidance_scale": 1.5,
                "delta": 1.0, "t_index_list": [10, 30]}

    def stats(self):
        return {}


def run(coro, timeout=30):
    loop = asyncio.new_event_loop()
    try:
        return loop.run_until_complete(asyncio.wait_for(coro, timeout))
    finally:
        loop.close()


def test_proxies_address_their_own_slot():
    async def body():
        base = RecordingPipeline()
        bp = BatchedPipeline(base, 2)
        a, b = bp.acquire("a"), bp.acquire("b")
        assert (a.slot, b.slot) == (0, 1)
        assert base.log == [("reset", 0), ("reset", 1)]
        base.log.clear()
        a.update_prompt("A")
        b.update_prompt("B")
        b.update_negative_prompt("N")
        a.update_guidance(2.0, 0.5)
        b.update_t_index_list([5, 45])
        assert base.log == [
            ("prompt", "A", 0), ("prompt", "B", 1),
            ("negative_prompt", "N", 1), ("guidance", 2.0, 0.5, 0),
            ("t_index_list", [5, 45], 1)]
        base.log.clear()
        bp.update_prompt("all")  # the broadcast path stays replica-wide
        bp.update_guidance(3.0)
        assert base.log == [("prompt", "all", None), ("guidance", 3.0, None, None)]
        per = bp.stats()["per_stream"]
        assert per[1]["prompt"] == "p1" and per[0]["t_index_list"] == [10, 30]
        assert {"negative_prompt", "guidance_scale", "delta"} <= set(per[0])
        # release + acquire hands the slot out reset
        base.log.clear()
        bp.release("b")
        c = bp.acquire("c")
        assert c.slot == 1 and base.log == [("reset", 1)]
        assert bp.acquire("c").slot == 1 and base.log == [("reset", 1)]
        bp.release("a")
        bp.release("c")

    run(body())


def test_acquire_resets_a_real_engine_slot():
    async def body():
        class Pipe:  # StreamDiffusionPipeline's surface over a tiny engine
            def __init__(self):
                self.engine = make_engine()
                self.cfg = self.engine.cfg
                for name in ("update_prompt", "reset_slot", "slot_controls", "stats"):
                    setattr(self, name, getattr(self.engine, name))

        bp = BatchedPipeline(Pipe(), 2)
        bp.acquire("a")
        b = bp.acquire("b")
        b.update_prompt(PROMPT_B)
        assert bp.stats()["per_stream"][1]["prompt"] == PROMPT_B
        bp.release("b")
        bp.acquire("c")
        per = bp.stats()["per_stream"]
        assert per[1]["prompt"] == per[0]["prompt"] == bp.cfg.prompt
        bp.release("a")
        bp.release("c")

    run(body())


OFFER_SDP = "\r\n".join([
    "v=0", "o=- 1 2 IN IP4 127.0.0.1", "s=-", "t=0 0",
    "m=video 51000 UDP/TLS/RTP/SAVPF 97",
    "a=ice-ufrag:abcd", "a=ice-pwd:efghijklmnop", "a=mid:0", "a=sendrecv",
    "a=rtpmap:97 H264/90000",
    "a=candidate:1 1 udp 2130706431 127.0.0.1 51000 typ host",
]) + "\r\n"


def test_config_route_addresses_sessions():
    async def body():
        base = RecordingPipeline()
        pool = PipelinePool([BatchedPipeline(base, 2)])
        client = TestClient(TestServer(create_app(pool=pool, use_turn=False)))
        await client.start_server()
        sids = []
        for _ in range(2):
            r = await client.post("/whip", data=OFFER_SDP,
                                  headers={"Content-Type": "application/sdp"})
            assert r.status == 201
            sids.append(r.headers["Location"].rsplit("/", 1)[1])
        slot1 = pool.stats()["per_replica"][0]  # both sessions on replica 0
        assert slot1["active_streams"] == 2
        base.log.clear()

        r = await client.post("/config", json={
            "stream_id": sids[1], "prompt": "mine", "negative_prompt": "n",
            "guidance_scale": 2, "delta": 0.5, "t_index_list": [5, 45]})
        assert r.status == 200
        assert base.log == [
            ("t_index_list", [5, 45], 1), ("prompt", "mine", 1),
            ("negative_prompt", "n", 1), ("guidance", 2.0, 0.5, 1)]
        base.log.clear()

        r = await client.post("/config", json={"stream_id": "nope", "prompt": "x"})
        assert r.status == 404 and base.log == []

        r = await client.post("/config", json={"prompt": "everyone", "delta": 0.25})
        assert r.status == 200
        assert base.log == [("prompt", "everyone", None),
                            ("guidance", None, 0.25, None)]
        base.log.clear()

        for bad in ({"guidance_scale": "strong"}, {"delta": [1]},
                    {"guidance_scale": True}, {"prompt": 5},
                    {"t_index_list": "10,30"}, {"t_index_list": [1.5, 2]},
                    {"stream_id": sids[0], "t_index_list": [10]},
                    {"stream_id": sids[0], "guidance_scale": None, "delta": "x"}):
            r = await client.post("/config", json=bad)
            assert r.status == 400, bad
        r = await client.post("/config", data="not json")
        assert r.status == 400
        assert base.log == []

        # a closed session's id is gone
        r = await client.delete(f"/whip/{sids[1]}")
        assert r.status == 200
        r = await client.post("/config", json={"stream_id": sids[1], "prompt": "x"})
        assert r.status == 404
        await client.close()

    run(body())


def test_datachannel_config_is_per_session_and_ignores_bad_values():
    base = RecordingPipeline()
    bp = BatchedPipeline(base, 2)

    async def body():
        a, b = bp.acquire("a"), bp.acquire("b")
        base.log.clear()
        _apply_session_config(b, {"prompt": "B", "guidance_scale": 2.5})
        _apply_session_config(a, {"guidance_scale": "strong"})  # logged, ignored
        _apply_session_config(a, {"t_index_list": [10]})        # wrong length
        _apply_session_config(a, "garbage")
        assert base.log == [("prompt", "B", 1), ("guidance", 2.5, None, 1)]
        bp.release("a")
        bp.release("b")

    run(body())
