"""YUV 4:2:0 (I420) frames without a GPU: the torch integer reference
against the C++ codec's own colour arithmetic, the codec's plane I/O, the
codec HAL and the CPU engine.

Everything is integer arithmetic, so every comparison is exact (tolerance 0).
The independent reference below (ref_rgb_to_i420 / ref_i420_to_rgb) is
written in numpy straight from the formulas and checks ops' torch reference
as well as the codec.
"""
import numpy as np
import pytest
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import EngineConfig
from ai_rtc_agent_amd.engine import StreamDiffusionEngine
from ai_rtc_agent_amd.media.codec import H264SwCodec, SoftwareCodec

ext = ops.hip_ext()
needs_ext = pytest.mark.skipif(
    ext is None or not hasattr(ext, "H264SwEncoder"),
    reason="native extension not built")


# ---------------------------------------------------------------------------
# independent reference (numpy int64; >> on negatives is arithmetic)
# ---------------------------------------------------------------------------
def _clip8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def ref_rgb_to_i420(rgb: torch.Tensor) -> torch.Tensor:
    p = rgb.numpy().astype(np.int64)
    h, w, _ = p.shape
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = _clip8(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16)
    m = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    r, g, b = m[..., 0], m[..., 1], m[..., 2]
    cb = _clip8(((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128)
    cr = _clip8(((112 * r - 94 * g - 18 * b + 128) >> 8) + 128)
    flat = np.concatenate([y.ravel(), cb.ravel(), cr.ravel()])
    return torch.from_numpy(flat.reshape(h * 3 // 2, w).copy())


def ref_i420_to_rgb(i420: torch.Tensor) -> torch.Tensor:
    rows, w = i420.shape
    h = rows * 2 // 3
    flat = i420.numpy().astype(np.int64).ravel()
    n, nc = h * w, (h // 2) * (w // 2)
    c = flat[:n].reshape(h, w) - 16
    d = (flat[n:n + nc].reshape(h // 2, w // 2) - 128).repeat(2, 0).repeat(2, 1)
    e = (flat[n + nc:].reshape(h // 2, w // 2) - 128).repeat(2, 0).repeat(2, 1)
    out = np.stack([
        _clip8((298 * c + 409 * e + 128) >> 8),
        _clip8((298 * c - 100 * d - 208 * e + 128) >> 8),
        _clip8((298 * c + 516 * d + 128) >> 8)], axis=-1)
    return torch.from_numpy(out.copy())


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------
def noise(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)


def primaries(h, w):
    """Saturated primaries/secondaries/black/white in 2-px-wide stripes
    whose phase shifts every other row, so 2x2 blocks mix colours too."""
    cols = torch.tensor([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0],
                         [0, 255, 255], [255, 0, 255], [0, 0, 0],
                         [255, 255, 255]], dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return cols[((xx + yy // 2) // 2 + yy // 3) % 8].contiguous()


def grey_ramp(h, w):
    v = (torch.arange(h * w) % 256).to(torch.uint8).reshape(h, w, 1)
    return v.expand(h, w, 3).contiguous()


def frames_for(h, w):
    return [noise(h, w, 1), noise(h, w, 2), primaries(h, w), grey_ramp(h, w)]


def as_bytes(t):
    return t.contiguous().numpy().tobytes()


SIZES = [(16, 16), (64, 48), (176, 144)]  # (w, h)
PAD_SIZES = [(20, 12), (50, 38)]          # not multiples of 16
ENC_MODES = [(1, 0), (1, 2), (4, 0), (4, 2)]  # (slices, mb_mode)
QP = 26


def edge_equal(f):
    """Make the last two columns and the last two rows equal: then the
    codec's clamped 2x2 mean over the padding equals plane-edge
    replication, and both entry points see the same padded planes."""
    f = f.clone()
    f[:, -2] = f[:, -1]
    f[-2, :] = f[-1, :]
    assert torch.equal(f[:, -2], f[:, -1]) and torch.equal(f[-2], f[-1])
    return f


def smooth(h, w, seed):
    """Gentle gradients: codes with a small error, so unchanged macroblocks
    of a following P frame fall under the encoder's skip threshold."""
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    ch = [(40 + seed + 2 * xx + yy) % 256, (200 - xx - 2 * yy) % 256,
          (90 + xx + yy) % 256]
    return torch.stack(ch, dim=-1).to(torch.uint8).contiguous()


def ipp_sequence(h, w, seed, prep=lambda f: f):
    """I, P, P over a smooth picture: frames 2 and 3 each replace one 16x16
    region by noise, so P_Skip and intra-refresh macroblocks both occur."""
    f0 = prep(smooth(h, w, seed))
    f1 = f0.clone()
    f1[:16, :16] = noise(16, 16, seed + 1)[:min(16, h), :min(16, w)]
    f2 = f1.clone()
    rh, rw = min(16, h), min(16, w)
    f2[h - rh:, w - rw:] = noise(rh, rw, seed + 2)
    return [f0, prep(f1), prep(f2)]


# ---------------------------------------------------------------------------
# the torch reference itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(2, 2), (2, 8), (6, 10), (38, 50), (48, 64)])
def test_torch_reference_matches_formulas(hw):
    h, w = hw
    for f in frames_for(h, w):
        i = ops.rgb_u8_to_i420(f)
        assert i.shape == (h * 3 // 2, w) and i.dtype == torch.uint8
        assert torch.equal(i, ref_rgb_to_i420(f))
        assert torch.equal(ops.i420_to_rgb_u8(i), ref_i420_to_rgb(i))
        assert torch.equal(ops.i420_to_rgb_u8(i, H=h), ref_i420_to_rgb(i))
    # batch == per-frame
    fs = torch.stack(frames_for(h, w))
    ib = ops.rgb_u8_to_i420(fs)
    assert ib.shape == (4, h * 3 // 2, w)
    for k in range(4):
        assert torch.equal(ib[k], ref_rgb_to_i420(fs[k]))
        assert torch.equal(ops.i420_to_rgb_u8(ib)[k], ref_i420_to_rgb(ib[k]))
    assert ops.is_i420(ib) and ops.is_i420(ib[0]) and not ops.is_i420(fs[0])
    assert ops.i420_size(ib) == (h, w) and ops.i420_size(ib[0]) == (h, w)


def test_i420_to_rgb_reference_all_clips():
    vals = [0, 16, 128, 235, 240, 255]
    combos = [(y, cb, cr) for y in vals for cb in vals for cr in vals]
    # one 2x2 block per combination, blocks side by side: (2, 2*216)
    n = len(combos)
    y = torch.tensor([c[0] for c in combos], dtype=torch.uint8)
    yp = y.repeat_interleave(2).repeat(2)                      # 2 rows
    cb = torch.tensor([c[1] for c in combos], dtype=torch.uint8)
    cr = torch.tensor([c[2] for c in combos], dtype=torch.uint8)
    i = torch.cat([yp, cb, cr]).reshape(3, 2 * n)
    got = ops.i420_to_rgb_u8(i)
    assert torch.equal(got, ref_i420_to_rgb(i))
    assert int(got.min()) == 0 and int(got.max()) == 255  # clips fired


def test_postprocess_to_i420_cpu_composes():
    g = torch.Generator().manual_seed(3)
    x = torch.rand((2, 6, 10, 3), generator=g) * 3 - 1.5
    want = ops.rgb_u8_to_i420(ops.postprocess_to_u8(x))
    assert torch.equal(ops.postprocess_to_i420(x), want)
    assert torch.equal(ops.postprocess_to_i420(x[0]), want[0])


# ---------------------------------------------------------------------------
# encode side: Python reference vs the C++ codec
# ---------------------------------------------------------------------------
@needs_ext
@pytest.mark.parametrize("mode", ENC_MODES, ids=lambda m: f"s{m[0]}m{m[1]}")
@pytest.mark.parametrize("wh", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_yuv_byte_identical(wh, mode):
    w, h = wh
    s, m = mode
    for f in frames_for(h, w):
        a = ext.H264SwEncoder(w, h, s, m).encode(as_bytes(f), QP)
        b = ext.H264SwEncoder(w, h, s, m).encode_yuv(
            as_bytes(ref_rgb_to_i420(f)), QP)
        assert a == b


def _encode_seq(w, h, s, m, frames, yuv):
    enc = ext.H264SwEncoder(w, h, s, m)
    out = []
    for k, f in enumerate(frames):
        if yuv:
            out.append(enc.encode_yuv(as_bytes(ref_rgb_to_i420(f)), QP,
                                      keyframe=(k == 0)))
        else:
            out.append(enc.encode(as_bytes(f), QP, keyframe=(k == 0)))
    return out


@needs_ext
@pytest.mark.parametrize("mode", ENC_MODES, ids=lambda m: f"s{m[0]}m{m[1]}")
@pytest.mark.parametrize("wh", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_yuv_ipp_sequence_byte_identical(wh, mode):
    w, h = wh
    frames = ipp_sequence(h, w, seed=10)
    a = _encode_seq(w, h, *mode, frames, yuv=False)
    b = _encode_seq(w, h, *mode, frames, yuv=True)
    assert a == b
    if (w, h) != (16, 16):
        # most macroblocks of the P frames are skipped: far smaller than the
        # same pictures coded as IDR
        s, m = mode
        for k in (1, 2):
            idr = ext.H264SwEncoder(w, h, s, m).encode(as_bytes(frames[k]), QP)
            assert len(a[k]) < len(idr)


@needs_ext
@pytest.mark.parametrize("mode", ENC_MODES, ids=lambda m: f"s{m[0]}m{m[1]}")
@pytest.mark.parametrize("wh", PAD_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_yuv_identity_with_padding(wh, mode):
    w, h = wh
    s, m = mode
    for f in frames_for(h, w):
        f = edge_equal(f)
        a = ext.H264SwEncoder(w, h, s, m).encode(as_bytes(f), QP)
        b = ext.H264SwEncoder(w, h, s, m).encode_yuv(
            as_bytes(ref_rgb_to_i420(f)), QP)
        assert a == b
    frames = ipp_sequence(h, w, seed=20, prep=edge_equal)
    assert _encode_seq(w, h, s, m, frames, False) == \
        _encode_seq(w, h, s, m, frames, True)


@needs_ext
def test_encode_yuv_rejects_bad_input():
    enc = ext.H264SwEncoder(16, 16, 1, 0)
    with pytest.raises(RuntimeError):
        enc.encode_yuv(b"\0" * (16 * 16 * 3), QP)      # RGB-sized buffer
    with pytest.raises(RuntimeError):
        ext.H264SwEncoder(17, 16, 1, 0).encode_yuv(b"\0" * (17 * 16 * 3 // 2), QP)


# ---------------------------------------------------------------------------
# decode side
# ---------------------------------------------------------------------------
def _i420_from(r, w, h):
    buf, dw, dh, is_i420 = r
    assert (dw, dh) == (w, h) and is_i420 is True
    assert len(buf) == w * h * 3 // 2
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).reshape(h * 3 // 2, w)


def _rgb_from(r, w, h):
    buf, dw, dh = r[:3]
    assert (dw, dh) == (w, h)
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).reshape(h, w, 3)


@needs_ext
@pytest.mark.parametrize("wh", SIZES + PAD_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_yuv_matches_decode(wh):
    w, h = wh
    for s, m in ((1, 0), (4, 2)):
        for f in frames_for(h, w):
            au = ext.H264SwEncoder(w, h, s, m).encode(as_bytes(f), QP)
            rgb = _rgb_from(ext.H264SwDecoder().decode(au), w, h)
            i420 = _i420_from(ext.H264SwDecoder().decode_yuv(au), w, h)
            assert torch.equal(ref_i420_to_rgb(i420), rgb)


@needs_ext
@pytest.mark.parametrize("wh", [(64, 48), (50, 38)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_mixed_calls_share_state(wh):
    w, h = wh
    frames = ipp_sequence(h, w, seed=30) + ipp_sequence(h, w, seed=31)[1:]
    aus = _encode_seq(w, h, 4, 2, frames, yuv=False)
    plain, mixed = ext.H264SwDecoder(), ext.H264SwDecoder()
    for k, au in enumerate(aus):
        want = _rgb_from(plain.decode(au), w, h)
        if k % 2:
            got = _rgb_from(mixed.decode(au), w, h)
        else:
            got = ref_i420_to_rgb(_i420_from(mixed.decode_yuv(au), w, h))
        assert torch.equal(got, want), f"picture {k} diverged"


@needs_ext
def test_decode_yuv_odd_size_returns_rgb():
    """decode_yuv hands a picture with an odd width or height out as RGB.
    The encoder crops in the SPS, whose unit for 4:2:0 is two luma samples,
    so the 18x10 stream decodes to an even size and is I420; an odd size
    cannot be produced by this encoder, and then the RGB branch has no
    stream to run on."""
    w, h = 18, 10
    au = ext.H264SwEncoder(w, h, 1, 0).encode(as_bytes(noise(h, w, 4)), QP)
    r = ext.H264SwDecoder().decode_yuv(au)
    assert r is not None
    _, dw, dh, is_i420 = r
    assert is_i420 is (dw % 2 == 0 and dh % 2 == 0)
    if is_i420:
        rgb = _rgb_from(ext.H264SwDecoder().decode(au), dw, dh)
        assert torch.equal(ref_i420_to_rgb(_i420_from(r, dw, dh)), rgb)
        pytest.skip(f"the {w}x{h} stream decodes to {dw}x{dh}: SPS cropping "
                    "is in units of two luma samples, the encoder cannot "
                    "make an odd-size stream")
    assert torch.equal(_rgb_from(r, dw, dh),
                       _rgb_from(ext.H264SwDecoder().decode(au), dw, dh))


# ---------------------------------------------------------------------------
# codec HAL
# ---------------------------------------------------------------------------
@needs_ext
def test_h264sw_codec_yuv_roundtrip():
    f = noise(48, 64, 5)
    i420 = ref_rgb_to_i420(f)
    c = H264SwCodec(yuv=True)
    data = c.encode(i420, keyframe=True)
    out = c.decode(data)
    assert out.shape == (72, 64) and out.dtype == torch.uint8 and ops.is_i420(out)
    # the same access unit as the RGB route, decoded without conversion
    plain = H264SwCodec()
    assert plain.encode(f, keyframe=True) == data
    rgb = plain.decode(data)
    assert rgb.shape == (48, 64, 3)
    assert torch.equal(ref_i420_to_rgb(out), rgb)
    # a yuv codec still takes RGB frames
    assert H264SwCodec(yuv=True).encode(f, keyframe=True) == data


@needs_ext
def test_h264sw_codec_default_unchanged():
    f = noise(48, 64, 6)
    c = H264SwCodec()
    assert c.yuv is False
    out = c.decode(c.encode(f, keyframe=True))
    assert out.shape == (48, 64, 3) and out.dtype == torch.uint8
    want = _rgb_from(ext.H264SwDecoder().decode(
        ext.H264SwEncoder(64, 48, 4, 2).encode(as_bytes(f), 30)), 64, 48)
    assert torch.equal(out, want)


def test_software_codec_takes_i420():
    i420 = ref_rgb_to_i420(noise(12, 20, 7))
    c = SoftwareCodec()
    out = c.decode(c.encode(i420, keyframe=True))
    assert torch.equal(out, ref_i420_to_rgb(i420))


def test_select_codec_follows_env(monkeypatch):
    from ai_rtc_agent_amd import config
    from ai_rtc_agent_amd.media.codec import select_codec

    monkeypatch.delenv("AIRTC_MEDIA_YUV", raising=False)
    assert config.media_yuv() is False
    assert EngineConfig().output_format == "rgb"
    assert getattr(select_codec(role="decode"), "yuv", False) is False
    monkeypatch.setenv("AIRTC_MEDIA_YUV", "1")
    assert config.media_yuv() is True
    assert EngineConfig().output_format == "i420"
    c = select_codec(role="decode")
    if isinstance(c, H264SwCodec):
        assert c.yuv is True
    with pytest.raises(ValueError):
        EngineConfig(output_format="nv12")


# ---------------------------------------------------------------------------
# engine on CPU
# ---------------------------------------------------------------------------
def make_engine(cfg, **kw):
    for k, v in kw.items():
        setattr(cfg, k, v)
    e = StreamDiffusionEngine(cfg)
    e.prepare()
    return e


def test_engine_cpu_i420_input(tiny_cfg):
    f = noise(64, 64, 8)
    i420 = ref_rgb_to_i420(f)
    a = make_engine(tiny_cfg)(i420)
    assert a.shape == (64, 64, 3)
    e = make_engine(tiny_cfg)
    b = e(ref_i420_to_rgb(i420))
    assert torch.equal(a, b)
    # an engine that has only ever seen RGB keeps its ingest record as it was
    assert "source_format" not in e.stats()["ingest"]
    # another size goes through the fit path, as its RGB conversion does
    small = ref_rgb_to_i420(noise(36, 48, 9))
    e1, e2 = make_engine(tiny_cfg), make_engine(tiny_cfg)
    assert torch.equal(e1(small), e2(ref_i420_to_rgb(small)))
    ing = e1.stats()["ingest"]
    assert ing["source_format"] == ["i420"] and ing["last_source_size"] == [[36, 48]]


def test_engine_cpu_i420_batch_and_list(tiny_cfg):
    tiny_cfg.frame_buffer_size = 2
    f = [noise(64, 64, 10), noise(64, 64, 11)]
    i = [ref_rgb_to_i420(x) for x in f]
    back = [ref_i420_to_rgb(x) for x in i]
    want = make_engine(tiny_cfg)(torch.stack(back))
    assert torch.equal(make_engine(tiny_cfg)(torch.stack(i)), want)
    e = make_engine(tiny_cfg)
    assert torch.equal(e([i[0], back[1]]), want)  # formats mixed in a list
    assert e.stats()["ingest"]["source_format"] == ["i420", "rgb"]


def test_engine_cpu_i420_output(tiny_cfg):
    f = noise(64, 64, 12)
    rgb = make_engine(tiny_cfg)(f)
    out = make_engine(tiny_cfg, output_format="i420")(f)
    assert out.shape == (96, 64) and out.dtype == torch.uint8
    assert torch.equal(out, ref_rgb_to_i420(rgb))


def test_engine_i420_output_needs_even_size(tiny_cfg):
    tiny_cfg.height = 63
    tiny_cfg.output_format = "i420"
    with pytest.raises(ValueError):
        StreamDiffusionEngine(tiny_cfg)


# ---------------------------------------------------------------------------
# error paths
# ---------------------------------------------------------------------------
def test_error_paths():
    u8 = torch.uint8
    with pytest.raises(ValueError):
        ops.rgb_u8_to_i420(torch.zeros((5, 4, 3), dtype=u8))       # odd H
    with pytest.raises(ValueError):
        ops.rgb_u8_to_i420(torch.zeros((4, 5, 3), dtype=u8))       # odd W
    with pytest.raises(ValueError):
        ops.rgb_u8_to_i420(torch.zeros((4, 4, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.rgb_u8_to_i420(torch.zeros((4, 4), dtype=u8))          # not RGB
    with pytest.raises(ValueError):
        ops.postprocess_to_i420(torch.zeros((3, 4, 3)))            # odd H
    with pytest.raises(ValueError):
        ops.postprocess_to_i420(torch.zeros((4, 4, 3), dtype=u8))  # not float
    with pytest.raises(ValueError):
        ops.i420_to_rgb_u8(torch.zeros((6, 5), dtype=u8))          # odd W
    with pytest.raises(ValueError):
        ops.i420_to_rgb_u8(torch.zeros((4, 4), dtype=u8))          # rows % 3
    with pytest.raises(ValueError):
        ops.i420_to_rgb_u8(torch.zeros((6, 4), dtype=torch.int16))
    with pytest.raises(ValueError):
        ops.i420_to_rgb_u8(torch.zeros((4, 4, 3), dtype=u8))       # RGB, 3-D
    with pytest.raises(ValueError):
        ops.i420_to_rgb_u8(torch.zeros((6, 4), dtype=u8), H=6)     # H is 4
    with pytest.raises(ValueError):
        ops.i420_size(torch.zeros((4, 4, 3), dtype=u8))
    assert not ops.is_i420(torch.zeros((6, 4), dtype=torch.float32))
