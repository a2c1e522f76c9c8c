"""HTTP signalling server + CLI — API parity with the reference agent.

Route table (reference agent.py:466-472):
    POST/DELETE /whip    publish via WHIP (SDP in/out, 201 + Location)
    POST/DELETE /whep    subscribe via WHEP (401 until a publisher exists)
    POST /offer          browser round-trip mode (JSON sdp exchange)
    POST /config         runtime {prompt, t_index_list} updates
    GET  /               health "OK" (polled by the runpod handler)
    GET  /stats          FPS + per-stage latency (ours; SURVEY.md §5.5 gap)

CLI flags mirror reference agent.py:441-455: --model-id --port --udp-ports
--log-level (+ MI355X extras: --gpus, --family, --resolution, --fit).

Session model: connection handling is identical to the reference at the
signalling level; the media transport underneath is our ICE-lite RTP stack
(media/rtc.py — see its DTLS note). Multi-GPU serving assigns each new
session to a pipeline replica (parallel/dispatch.py), replacing the
reference's single shared pipeline (agent.py:423).
"""
from __future__ import annotations

import argparse
import logging
import math
import os
import uuid
from typing import Optional

from aiohttp import web

from .engine import LORA_KEEP
from .media.ice import get_ice_servers, get_link_headers
from .media.rtc import MediaRelay, PeerConnection, set_udp_port_pool
from .media.tracks import VideoStreamTrack
from .utils.events import StreamEventHandler

logger = logging.getLogger(__name__)


def _state(app: web.Application) -> dict:
    return app["state"]


async def offer(request: web.Request) -> web.Response:
    """Browser round-trip: same PC receives source video and sends the
    stylised stream back (reference agent.py:123-208)."""
    params = await request.json()
    room_id = params.get("room_id")
    stream_id = str(uuid.uuid4())
    st = _state(request.app)

    pc = PeerConnection(ice_servers=st["ice_servers"])
    st["pcs"].add(pc)
    pipeline = st["pool"].assign(stream_id)
    st.setdefault("session_pipelines", {})[stream_id] = pipeline
    events: StreamEventHandler = st["events"]

    @pc.on("datachannel_message")
    def on_config(msg: dict) -> None:
        _apply_session_config(pipeline, msg)

    @pc.on("track")
    def on_track(track) -> None:
        logger.info("track received for stream %s", stream_id)
        video = VideoStreamTrack(track, pipeline)
        pc.add_track(video)

    @pc.on("connectionstatechange")
    async def on_state() -> None:
        logger.info("pc state %s (stream %s)", pc.connection_state, stream_id)
        if pc.connection_state == "connected":
            await events.stream_started(stream_id, room_id)
        elif pc.connection_state in ("failed", "closed"):
            st["pcs"].discard(pc)
            st["pool"].release(stream_id)
            st.get("session_pipelines", {}).pop(stream_id, None)
            if pc.connection_state == "closed":
                await events.stream_ended(stream_id, room_id)

    await pc.set_remote_description(params["offer"]["sdp"])
    sdp = await pc.create_answer(host=request.app["host"])
    return web.json_response({"sdp": sdp, "type": "answer"})


async def whip(request: web.Request) -> web.Response:
    """WHIP publish: ingests the source; output is consumed via /whep
    (reference agent.py:285-395 — note whip does NOT send video back)."""
    offer_sdp = await request.text()
    st = _state(request.app)
    stream_id = str(uuid.uuid4())

    # No TURN on WHIP: OBS does not trickle ICE (reference comment
    # agent.py:299-315), so the answer carries only host candidates.
    pc = PeerConnection()
    st["pcs"].add(pc)
    pipeline = st["pool"].assign(stream_id)
    st.setdefault("session_pipelines", {})[stream_id] = pipeline
    events: StreamEventHandler = st["events"]

    @pc.on("datachannel_message")
    def on_config(msg: dict) -> None:
        _apply_session_config(pipeline, msg)

    @pc.on("track")
    def on_track(track) -> None:
        st["source_track"] = VideoStreamTrack(track, pipeline)
        logger.info("whip publisher track stored (stream %s)", stream_id)

    @pc.on("connectionstatechange")
    async def on_state() -> None:
        if pc.connection_state == "connected":
            await events.stream_started(stream_id)
        elif pc.connection_state in ("failed", "closed"):
            st["pcs"].discard(pc)
            st["pool"].release(stream_id)
            st.get("session_pipelines", {}).pop(stream_id, None)
            if st.get("whip_pc") is pc:
                st["source_track"] = None
                st["whip_pc"] = None
            if pc.connection_state == "closed":
                await events.stream_ended(stream_id)

    st["whip_pc"] = pc
    st.setdefault("whip_sessions", {})[stream_id] = pc
    await pc.set_remote_description(offer_sdp)
    sdp = await pc.create_answer(host=request.app["host"], direction="recvonly")
    # per-session resource URL (the WHIP spec's DELETE target; OBS follows
    # the Location header). Bare DELETE /whip still closes the current
    # publisher for reference-parity clients.
    headers = {"Location": f"/whip/{stream_id}"}
    for link in get_link_headers(st["ice_servers"]):
        headers.setdefault("Link", link)
    return web.Response(status=201, content_type="application/sdp", text=sdp, headers=headers)


async def whip_delete(request: web.Request) -> web.Response:
    st = _state(request.app)
    sid = request.match_info.get("sid")
    if sid is not None:
        pc = st.get("whip_sessions", {}).pop(sid, None)
        if pc is None:
            return web.Response(status=404)
        await pc.close()
        if st.get("whip_pc") is pc:
            st["whip_pc"] = None
            st["source_track"] = None
        st["pool"].release(sid)
        st.get("session_pipelines", {}).pop(sid, None)
        return web.Response(status=200)
    pc = st.get("whip_pc")
    if pc is not None:
        await pc.close()
        st["whip_pc"] = None
        st["source_track"] = None
    return web.Response(status=200)


async def whep(request: web.Request) -> web.Response:
    """WHEP subscribe to the current publisher's stylised stream
    (reference agent.py:211-282; 401 without a publisher, :218-220)."""
    st = _state(request.app)
    if st.get("source_track") is None:
        return web.Response(status=401, text="no active publisher")
    offer_sdp = await request.text()

    pc = PeerConnection()
    st["pcs"].add(pc)
    st.setdefault("whep_pcs", set()).add(pc)
    # relay fan-out so N viewers share one pipeline pull (the reference
    # attaches the track directly and leaves its MediaRelay unused,
    # agent.py:248-252 — with >1 viewer they would steal frames from each
    # other; the relay fixes that)
    pc.add_track(st["relay"].subscribe(st["source_track"]))

    @pc.on("connectionstatechange")
    def on_state() -> None:
        if pc.connection_state in ("failed", "closed"):
            st["pcs"].discard(pc)
            st.get("whep_pcs", set()).discard(pc)

    await pc.set_remote_description(offer_sdp)
    sdp = await pc.create_answer(host=request.app["host"], direction="sendonly")
    return web.Response(
        status=201, content_type="application/sdp", text=sdp,
        headers={"Location": "/whep"},
    )


async def whep_delete(request: web.Request) -> web.Response:
    """Close every WHEP subscriber PC (the WHEP resource URL carries no
    per-session id in this minimal server, so DELETE tears down all)."""
    st = _state(request.app)
    for pc in list(st.get("whep_pcs", ())):
        await pc.close()
        st["pcs"].discard(pc)
        st["whep_pcs"].discard(pc)
    return web.Response(status=200)


def _checked_config(params) -> dict:
    """The recognised keys of a config message, type-checked; ValueError on
    a malformed value (HTTP answers 400, the datachannel logs and ignores)."""
    if not isinstance(params, dict):
        raise ValueError("config must be a JSON object")
    out = {}
    t = params.get("t_index_list")
    if t is not None:
        if (not isinstance(t, (list, tuple)) or not t
                or any(isinstance(v, bool) or not isinstance(v, int) for v in t)):
            raise ValueError("t_index_list must be a non-empty list of integers")
        out["t_index_list"] = list(t)
    for key in ("prompt", "negative_prompt"):
        v = params.get(key)
        if v is not None:
            if not isinstance(v, str):
                raise ValueError(f"{key} must be a string")
            out[key] = v
    for key in ("guidance_scale", "delta"):
        v = params.get(key)
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{key} must be a finite number")
            out[key] = float(v)
    for key in ("canny_low", "canny_high"):
        v = params.get(key)
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 2040:
                raise ValueError(f"{key} must be an integer in [0, 2040]")
            out[key] = v
    if "canny_low" in out and "canny_high" in out and out["canny_low"] > out["canny_high"]:
        raise ValueError("canny_low must not exceed canny_high")
    if "lora" in params:
        # a name the operator loaded, or null for no adapter: never a path or
        # a bank index
        v = params["lora"]
        if v is not None and (not isinstance(v, str) or not v):
            raise ValueError("lora must be the name of a loaded adapter or null")
        out["lora"] = v
    v = params.get("lora_scale")
    if v is not None:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError("lora_scale must be a finite number")
        out["lora_scale"] = float(v)
    return out


def _apply_config(pipeline, params: dict) -> None:
    """Shared by POST /config and the datachannel messages
    (reference agent.py:154-168, 324-337, 398-412). A session's datachannel
    hands in its own pipeline — for a batched replica its SlotProxy, so the
    update reaches that session alone. Raises ValueError on malformed
    values (including what the pipeline itself rejects, such as a
    per-session t_index_list of another length)."""
    _apply_checked(pipeline, _checked_config(params))


def _apply_checked(pipeline, cfg: dict) -> None:
    """Apply a type-checked config, key by key. The pipeline itself may
    still reject a value (ValueError): a per-session t_index_list of another
    length, a per-session guidance raise on an engine without
    runtime_guidance, a LoRA name nobody loaded (the slot keeps the adapter
    it had). Keys applied before the rejected one stay applied."""
    if "lora" in cfg or "lora_scale" in cfg:
        # first: the key most likely to be refused touches nothing else
        pipeline.update_lora(cfg.get("lora", LORA_KEEP), cfg.get("lora_scale"))
    if "t_index_list" in cfg:
        pipeline.update_t_index_list(cfg["t_index_list"])
    if "prompt" in cfg:
        pipeline.update_prompt(cfg["prompt"])
    if "negative_prompt" in cfg:
        pipeline.update_negative_prompt(cfg["negative_prompt"])
    if "guidance_scale" in cfg or "delta" in cfg:
        pipeline.update_guidance(cfg.get("guidance_scale"), cfg.get("delta"))
    if "canny_low" in cfg or "canny_high" in cfg:
        pipeline.update_canny(cfg.get("canny_low"), cfg.get("canny_high"))


def _apply_session_config(pipeline, msg) -> None:
    """Datachannel form: a malformed message is logged and ignored."""
    try:
        _apply_config(pipeline, msg)
    except ValueError as e:
        logger.warning("ignored config message: %s", e)


async def update_config(request: web.Request) -> web.Response:
    """POST /config. With "stream_id" (the id in the WHIP Location header)
    that session alone is updated — 404 when it is unknown; without it every
    active pipeline is. Malformed values answer 400: a wrong type before
    anything is touched, a value the pipeline rejects (_apply_checked) after
    the keys that precede it were applied."""
    try:
        params = await request.json()
    except ValueError:
        return web.json_response({"error": "body must be JSON"}, status=400)
    st = _state(request.app)
    sid = params.get("stream_id") if isinstance(params, dict) else None
    if sid is not None:
        targets = [st.get("session_pipelines", {}).get(sid)]
        if targets[0] is None:
            return web.json_response({"error": f"unknown stream_id {sid!r}"}, status=404)
    else:
        targets = st["pool"].active()
    try:
        cfg = _checked_config(params)  # reject before any pipeline is touched
        for pipeline in targets:
            _apply_checked(pipeline, cfg)
    except ValueError as e:
        return web.json_response({"error": str(e)}, status=400)
    return web.json_response({"status": "ok"})


async def health(request: web.Request) -> web.Response:
    return web.Response(text="OK")


async def stats(request: web.Request) -> web.Response:
    st = _state(request.app)
    return web.json_response(st["pool"].stats())


async def metrics(request: web.Request) -> web.Response:
    """Prometheus exposition of the /stats content (the
    reference has no metrics endpoint at all; /stats is the JSON form,
    this is the scrapeable one)."""
    st = _state(request.app)
    pool = st["pool"].stats()
    lines = [
        "# TYPE airtc_replicas gauge",
        f"airtc_replicas {pool.get('replicas', 0)}",
        "# TYPE airtc_sessions gauge",
        f"airtc_sessions {len(pool.get('sessions', {}))}",
        "# TYPE airtc_peer_connections gauge",
        f"airtc_peer_connections {len(st.get('pcs', ()))}",
        "# TYPE airtc_frames_total counter",
        "# TYPE airtc_fps gauge",
        "# TYPE airtc_stage_ms gauge",
    ]
    for i, rep in enumerate(pool.get("per_replica", [])):
        lines.append(f'airtc_frames_total{{replica="{i}"}} {rep.get("frames", 0)}')
        lines.append(f'airtc_fps{{replica="{i}"}} {rep.get("fps", 0.0)}')
        for stage, v in rep.get("stages_ms", {}).items():
            for q in ("p50", "p90"):
                lines.append(
                    f'airtc_stage_ms{{replica="{i}",stage="{stage}",q="{q}"}} '
                    f'{v.get(q, 0.0)}')
        for si, slot in enumerate(rep.get("per_stream", [])):
            if slot.get("p50_ms") is not None:
                lines.append(
                    f'airtc_stream_latency_ms{{replica="{i}",slot="{si}"}} '
                    f'{slot["p50_ms"]}')
    return web.Response(text="\n".join(lines) + "\n",
                        content_type="text/plain")


async def on_startup(app: web.Application) -> None:
    st = _state(app)
    if app["udp_ports"]:
        set_udp_port_pool(app["udp_ports"])
    from .parallel.dispatch import PipelinePool

    if st.get("pool") is None:
        from .config import EngineConfig

        cfg = EngineConfig(
            model_id=app["model_id"],
            model_family=app.get("family", "sd15"),
            width=app.get("resolution", 512),
            height=app.get("resolution", 512),
        )
        if app.get("fit_mode"):
            cfg.fit_mode = app["fit_mode"]
        if app.get("output_size"):
            cfg.output_size = app["output_size"]
        if app.get("output_max_side") is not None:
            cfg.output_max_side = app["output_max_side"]
        for key in ("controlnet_processor", "controlnet_scale", "canny_low",
                    "canny_high", "canny_reach"):
            if app.get(key) is not None:
                setattr(cfg, key, app[key])
        if cfg.controlnet_processor != "none":
            # a conditioning processor is only ever wanted with its ControlNet
            cfg.use_controlnet = True
        for key in ("safety_checker", "safety_adjustment"):
            if app.get(key) is not None:
                setattr(cfg, key, app[key])
        if app.get("safety_checker") or os.environ.get("AIRTC_SAFETY_CHECKER"):
            # naming a checker (flag or environment) switches the gate on
            cfg.use_safety_checker = True
        if app.get("full_vae"):
            cfg.use_tiny_vae = False
        for key in ("lora_adapters", "lora_max_rank"):
            if app.get(key) is not None:
                setattr(cfg, key, app[key])
        cfg.__post_init__()  # validate what was set after construction
        from .config import lora_adapter_specs

        specs = lora_adapter_specs(app.get("lora_adapter"))
        if len(specs) > cfg.lora_adapters:
            raise ValueError(
                f"{len(specs)} LoRA adapters named, the bank holds "
                f"{cfg.lora_adapters} (--lora-adapters)")
        st["pool"] = PipelinePool.create(
            model_id=app["model_id"], n_gpus=app["n_gpus"], cfg=cfg,
            streams_per_replica=app.get("streams_per_gpu", 1),
        )
        if specs:
            # the names a session may choose among (POST /config "lora")
            for p in st["pool"].active():
                p.load_adapters(specs)
    st["ice_servers"] = get_ice_servers() if app["use_turn"] else []


async def on_shutdown(app: web.Application) -> None:
    st = _state(app)
    for pc in list(st["pcs"]):
        await pc.close()
    st["pcs"].clear()


@web.middleware
async def cors_middleware(request: web.Request, handler):
    """CORS for browser clients (the reference pulls in aiohttp_middlewares'
    cors_middleware, agent.py:459; ours is self-contained)."""
    if request.method == "OPTIONS":
        resp = web.Response(status=204)
    else:
        resp = await handler(request)
    resp.headers["Access-Control-Allow-Origin"] = "*"
    resp.headers["Access-Control-Allow-Methods"] = "GET, POST, DELETE, OPTIONS"
    resp.headers["Access-Control-Allow-Headers"] = "Content-Type, Authorization"
    return resp


def create_app(
    model_id: str = "lykon/dreamshaper-8",
    udp_ports: Optional[list] = None,
    pool=None,
    host: str = "127.0.0.1",
    n_gpus: int = 1,
    use_turn: bool = True,
    family: str = "sd15",
    resolution: int = 512,
    streams_per_gpu: int = 1,
    fit_mode: Optional[str] = None,
    output_size: Optional[str] = None,
    output_max_side: Optional[int] = None,
    controlnet_processor: Optional[str] = None,
    controlnet_scale: Optional[float] = None,
    canny_low: Optional[int] = None,
    canny_high: Optional[int] = None,
    canny_reach: Optional[int] = None,
    safety_checker: Optional[str] = None,
    safety_adjustment: Optional[float] = None,
    full_vae: bool = False,
    lora_adapters: Optional[int] = None,
    lora_max_rank: Optional[int] = None,
    lora_adapter: Optional[list] = None,
) -> web.Application:
    app = web.Application(middlewares=[cors_middleware])
    app["model_id"] = model_id
    app["udp_ports"] = udp_ports
    app["host"] = host
    app["n_gpus"] = n_gpus
    app["use_turn"] = use_turn
    app["family"] = family
    app["resolution"] = resolution
    app["streams_per_gpu"] = streams_per_gpu
    app["fit_mode"] = fit_mode  # None: EngineConfig default (AIRTC_FIT_MODE)
    # None: EngineConfig defaults (AIRTC_OUTPUT_SIZE, AIRTC_OUTPUT_MAX_SIDE)
    app["output_size"] = output_size
    app["output_max_side"] = output_max_side
    # None: EngineConfig defaults (AIRTC_CONTROLNET_PROCESSOR, AIRTC_CANNY_*);
    # a processor other than "none" switches the ControlNet on
    app["controlnet_processor"] = controlnet_processor
    app["controlnet_scale"] = controlnet_scale
    app["canny_low"] = canny_low
    app["canny_high"] = canny_high
    app["canny_reach"] = canny_reach
    # None: EngineConfig defaults (AIRTC_SAFETY_CHECKER, AIRTC_SAFETY_ADJUSTMENT);
    # naming a checker switches the output gate on. Deliberately not part of
    # the runtime config: a publisher must not relax its own gate
    app["safety_checker"] = safety_checker
    app["safety_adjustment"] = safety_adjustment
    # False: EngineConfig default (AIRTC_TINY_VAE); True: the full AutoencoderKL
    app["full_vae"] = full_vae
    # None: EngineConfig defaults (AIRTC_LORA_ADAPTERS, AIRTC_LORA_MAX_RANK)
    # and $AIRTC_LORA_ADAPTER_FILES; NAME=PATH[:SCALE] strings otherwise
    app["lora_adapters"] = lora_adapters
    app["lora_max_rank"] = lora_max_rank
    app["lora_adapter"] = lora_adapter
    app["state"] = {
        "pcs": set(),
        "source_track": None,
        "whip_pc": None,
        "events": StreamEventHandler(),
        "relay": MediaRelay(),
        "pool": pool,
        "ice_servers": [],
    }
    app.router.add_post("/offer", offer)
    app.router.add_post("/whip", whip)
    app.router.add_delete("/whip", whip_delete)
    app.router.add_delete("/whip/{sid}", whip_delete)
    app.router.add_post("/whep", whep)
    app.router.add_delete("/whep", whep_delete)
    app.router.add_post("/config", update_config)
    app.router.add_get("/", health)
    app.router.add_get("/stats", stats)
    app.router.add_get("/metrics", metrics)
    app.on_startup.append(on_startup)
    app.on_shutdown.append(on_shutdown)
    return app


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="MI355X real-time video-diffusion agent")
    parser.add_argument("--model-id", default="lykon/dreamshaper-8")
    parser.add_argument("--port", type=int, default=8888)
    parser.add_argument("--udp-ports", default=None, help="e.g. 40000-40100")
    parser.add_argument("--log-level", default="INFO")
    parser.add_argument("--gpus", type=int, default=1, help="pipeline replicas (one per GPU)")
    parser.add_argument("--host", default="0.0.0.0")
    parser.add_argument("--family", default="sd15", choices=["sd15", "sd21", "sdxl"],
                        help="UNet family served by the pipeline")
    parser.add_argument("--resolution", type=int, default=512)
    parser.add_argument("--fit", default=None,
                        choices=["cover", "contain", "stretch"],
                        help="how frames of another size are fitted to "
                             "--resolution on the GPU: cover = centred crop "
                             "to the engine aspect then resize (default), "
                             "contain = whole frame with black bars, "
                             "stretch = whole frame, aspect not kept "
                             "(default: $AIRTC_FIT_MODE or cover)")
    parser.add_argument("--output-size", default=None,
                        choices=["engine", "source"],
                        help="size of the frames sent back: engine = "
                             "--resolution, as ever; source = each session "
                             "gets the size it publishes (contain loses its "
                             "bars, cover returns the part of the picture "
                             "that was used), resized on the GPU "
                             "(default: $AIRTC_OUTPUT_SIZE or engine)")
    parser.add_argument("--output-max-side", type=int, default=None,
                        help="with --output-size source: cap on the longer "
                             "side of a returned frame, aspect kept; the "
                             "software encoder's cost grows with the "
                             "outgoing pixel count (default: "
                             "$AIRTC_OUTPUT_MAX_SIDE or 0 = no cap)")
    parser.add_argument("--yuv", action="store_true",
                        help="exchange YUV 4:2:0 (I420) frames between the "
                             "codec and the engine instead of packed RGB: "
                             "colour conversion runs on the GPU and the "
                             "codec reads/writes its planes directly "
                             "(same as AIRTC_MEDIA_YUV=1)")
    parser.add_argument("--runtime-guidance", action="store_true",
                        help="keep the RCFG step in the captured graph "
                             "whatever the initial guidance_scale, so a "
                             "session can raise its guidance at runtime "
                             "(same as AIRTC_RUNTIME_GUIDANCE=1)")
    parser.add_argument("--controlnet-processor", default=None,
                        choices=["none", "canny"],
                        help="turn each live frame into the ControlNet's "
                             "hint: canny = edge map computed on the GPU "
                             "inside the captured graph, every in-flight "
                             "stage conditioned on its own frame; any value "
                             "but none switches the ControlNet on (default: "
                             "$AIRTC_CONTROLNET_PROCESSOR or none)")
    parser.add_argument("--controlnet-scale", type=float, default=None,
                        help="weight of the ControlNet residuals (default: "
                             "$AIRTC_CONTROLNET_SCALE or 1.0)")
    parser.add_argument("--canny-low", type=int, default=None,
                        help="lower hysteresis threshold on the L1 gradient "
                             "magnitude, 0..2040; per session at runtime via "
                             "POST /config (default: $AIRTC_CANNY_LOW or 100)")
    parser.add_argument("--canny-high", type=int, default=None,
                        help="upper hysteresis threshold "
                             "(default: $AIRTC_CANNY_HIGH or 200)")
    parser.add_argument("--canny-reach", type=int, default=None,
                        help="how many 3x3 steps a weak edge may lie from a "
                             "strong one, 0..32; cv2.Canny's hysteresis is "
                             "unbounded (default: $AIRTC_CANNY_REACH or 16)")
    parser.add_argument("--safety-checker", default=None,
                        choices=["tiny", "clip"],
                        help="gate every returned frame with a safety "
                             "checker and send black for a flagged one: "
                             "clip = the CLIP ViT-L/14 "
                             "StableDiffusionSafetyChecker, run inside the "
                             "captured decode graph; tiny = the small conv "
                             "classifier (default: $AIRTC_SAFETY_CHECKER, "
                             "else no checker)")
    parser.add_argument("--full-vae", action="store_true",
                        help="decode and encode with the checkpoint's full "
                             "AutoencoderKL instead of TAESD: sharper frames "
                             "at about a third of the frame rate; sd15 / sd21 "
                             "only (default: $AIRTC_TINY_VAE=0 asks for it "
                             "too)")
    parser.add_argument("--safety-adjustment", type=float, default=None,
                        help="added to every clip checker score, positive is "
                             "stricter; operator-only, not reachable from "
                             "POST /config (default: "
                             "$AIRTC_SAFETY_ADJUSTMENT or 0)")
    parser.add_argument("--lora-adapters", type=int, default=None,
                        help="capacity of the per-session LoRA bank, 0..64; "
                             "0 = off. Sessions of a batched replica then "
                             "choose their own adapter through POST /config "
                             "\"lora\" without a graph re-capture (default: "
                             "$AIRTC_LORA_ADAPTERS or 0)")
    parser.add_argument("--lora-max-rank", type=int, default=None,
                        help="largest adapter rank the bank accepts, 1..64 "
                             "(default: $AIRTC_LORA_MAX_RANK or 32)")
    parser.add_argument("--lora-adapter", action="append", default=None,
                        metavar="NAME=PATH[:SCALE]",
                        help="load this adapter file into the bank at "
                             "start-up under NAME; repeatable, at most "
                             "--lora-adapters of them. Clients choose among "
                             "these names and never supply a path (default: "
                             "$AIRTC_LORA_ADAPTER_FILES, comma-separated)")
    parser.add_argument("--streams-per-gpu", type=int, default=1,
                        help="multi-stream batched serving: sessions per "
                             "GPU batched through one engine (fbs=K; "
                             "profiles/batching_ab.md measured +124% "
                             "aggregate at K=8)")
    parser.add_argument("--workers", type=int, default=0,
                        help="process-per-GPU serving: spawn N worker agents "
                             "(one per GPU, own media sockets) behind a "
                             "signalling front-end (SURVEY.md §5.8); 0 = "
                             "single-process mode")
    return parser


def main() -> None:
    args = build_parser().parse_args()

    logging.basicConfig(level=getattr(logging, args.log_level.upper(), logging.INFO))
    if args.yuv:
        # read by config.media_yuv() (codec selection, EngineConfig's
        # output_format default) here and in spawned workers
        os.environ["AIRTC_MEDIA_YUV"] = "1"
    if args.runtime_guidance:
        # read by EngineConfig.runtime_guidance here and in spawned workers
        os.environ["AIRTC_RUNTIME_GUIDANCE"] = "1"
    ports = None
    if args.udp_ports:
        lo, _, hi = args.udp_ports.partition("-")
        ports = list(range(int(lo), int(hi or lo) + 1))
    if args.workers > 0:
        import asyncio

        import torch

        from .parallel.frontend import WorkerFrontend

        if args.fit:
            # workers are spawned processes: they inherit the environment
            # and EngineConfig.fit_mode defaults from it
            os.environ["AIRTC_FIT_MODE"] = args.fit
        if args.output_size:
            os.environ["AIRTC_OUTPUT_SIZE"] = args.output_size
        if args.output_max_side is not None:
            os.environ["AIRTC_OUTPUT_MAX_SIDE"] = str(args.output_max_side)
        for flag, env in (("controlnet_processor", "AIRTC_CONTROLNET_PROCESSOR"),
                          ("controlnet_scale", "AIRTC_CONTROLNET_SCALE"),
                          ("canny_low", "AIRTC_CANNY_LOW"),
                          ("canny_high", "AIRTC_CANNY_HIGH"),
                          ("canny_reach", "AIRTC_CANNY_REACH"),
                          ("safety_checker", "AIRTC_SAFETY_CHECKER"),
                          ("safety_adjustment", "AIRTC_SAFETY_ADJUSTMENT")):
            if getattr(args, flag) is not None:
                os.environ[env] = str(getattr(args, flag))
        if args.full_vae:
            os.environ["AIRTC_TINY_VAE"] = "0"
        for flag, env in (("lora_adapters", "AIRTC_LORA_ADAPTERS"),
                          ("lora_max_rank", "AIRTC_LORA_MAX_RANK")):
            if getattr(args, flag) is not None:
                os.environ[env] = str(getattr(args, flag))
        if args.lora_adapter:
            os.environ["AIRTC_LORA_ADAPTER_FILES"] = ",".join(args.lora_adapter)
        fe = WorkerFrontend(args.workers, model_id=args.model_id,
                            family=args.family, resolution=args.resolution,
                            pin_gpu=torch.cuda.is_available(),
                            udp_ports=ports)
        fe.spawn()
        asyncio.get_event_loop().run_until_complete(fe.wait_ready())
        try:
            web.run_app(fe.create_app(), host=args.host, port=args.port)
        finally:
            fe.shutdown()
        return
    app = create_app(model_id=args.model_id, udp_ports=ports, n_gpus=args.gpus,
                     family=args.family, resolution=args.resolution,
                     streams_per_gpu=args.streams_per_gpu, fit_mode=args.fit,
                     output_size=args.output_size,
                     output_max_side=args.output_max_side,
                     controlnet_processor=args.controlnet_processor,
                     controlnet_scale=args.controlnet_scale,
                     canny_low=args.canny_low, canny_high=args.canny_high,
                     canny_reach=args.canny_reach,
                     safety_checker=args.safety_checker,
                     safety_adjustment=args.safety_adjustment,
                     full_vae=args.full_vae,
                     lora_adapters=args.lora_adapters,
                     lora_max_rank=args.lora_max_rank,
                     lora_adapter=args.lora_adapter)
    web.run_app(app, host=args.host, port=args.port)


if __name__ == "__main__":
    main()
