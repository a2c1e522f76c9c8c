"""YUV 4:2:0 (I420) on the GPU: the three colour kernels against the torch
integer reference, bit-exact, and graph engines fed and returning I420.

Integer arithmetic throughout: every comparison is torch.equal.
"""
import pytest
import torch

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.config import sd_turbo_config
from ai_rtc_agent_amd.engine import StreamDiffusionEngine

from test_yuv_cpu import (grey_ramp, noise, primaries, ref_i420_to_rgb,
                          ref_rgb_to_i420)

pytestmark = pytest.mark.gpu

# a single chroma sample, a single vector block, a tail-only width, a batch
# of more than one vector block per row, a plain aligned case, and vector
# blocks plus a tail on rows whose alignment changes from row to row
SHAPES = [(1, 2, 2), (1, 2, 8), (1, 6, 10), (2, 4, 24), (3, 48, 64), (1, 38, 50)]


def shape_id(s):
    return "x".join(map(str, s))


def rgb_inputs(B, H, W):
    """seeded noise, the grey ramp, saturated corner colours"""
    return [torch.stack([noise(H, W, 100 + b) for b in range(B)]),
            torch.stack([grey_ramp(H, W)] * B),
            torch.stack([primaries(H, W)] * B)]


def ref_batch(fn, x):
    return torch.stack([fn(t) for t in x])


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_rgb_u8_to_i420_kernel(shape):
    B, H, W = shape
    for x in rgb_inputs(B, H, W):
        got = ops.rgb_u8_to_i420(x.cuda())
        assert got.shape == (B, H * 3 // 2, W) and got.dtype == torch.uint8
        assert torch.equal(got.cpu(), ref_batch(ref_rgb_to_i420, x))
    # unbatched form
    assert torch.equal(ops.rgb_u8_to_i420(x[0].cuda()).cpu(), ref_rgb_to_i420(x[0]))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_i420_to_rgb_u8_kernel(shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(7)
    planes = [torch.randint(0, 256, (B, H * 3 // 2, W), generator=g, dtype=torch.uint8),
              ref_batch(ref_rgb_to_i420, torch.stack([grey_ramp(H, W)] * B))]
    for x in planes:
        got = ops.i420_to_rgb_u8(x.cuda())
        assert got.shape == (B, H, W, 3) and got.dtype == torch.uint8
        assert torch.equal(got.cpu(), ref_batch(ref_i420_to_rgb, x))
    assert torch.equal(ops.i420_to_rgb_u8(x[0].cuda(), H=H).cpu(), ref_i420_to_rgb(x[0]))


def test_i420_to_rgb_u8_kernel_all_clips():
    """Every combination of Y, Cb, Cr in {0,16,128,235,240,255}: all three
    clips fire in both directions. One 2x2 block per combination."""
    vals = [0, 16, 128, 235, 240, 255]
    combos = [(y, cb, cr) for y in vals for cb in vals for cr in vals]
    n = len(combos)
    y = torch.tensor([c[0] for c in combos], dtype=torch.uint8)
    cb = torch.tensor([c[1] for c in combos], dtype=torch.uint8)
    cr = torch.tensor([c[2] for c in combos], dtype=torch.uint8)
    x = torch.cat([y.repeat_interleave(2).repeat(2), cb, cr]).reshape(3, 2 * n)
    want = ref_i420_to_rgb(x)
    assert int(want.min()) == 0 and int(want.max()) == 255
    assert torch.equal(ops.i420_to_rgb_u8(x.cuda()).cpu(), want)


def f16_images(B, H, W):
    """f16 values spanning [-1.5, 1.5], the first ones at the exact .5
    rounding points k/127.5 - 1 (k + 0.5 before rounding) and around them"""
    n = B * H * W * 3
    g = torch.Generator().manual_seed(11)
    x = torch.rand(n, generator=g) * 3 - 1.5
    k = torch.arange(n) % 256
    ties = (k.float() + 0.5) / 127.5 - 1.0
    exact = k.float() / 127.5 - 1.0
    x[0::3] = ties[0::3]
    x[1::3] = exact[1::3]
    return x.reshape(B, H, W, 3).to(torch.float16)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_postprocess_to_i420_kernel(shape):
    """postprocess_to_i420(x) == rgb_u8_to_i420(postprocess_to_u8(x)).
    postprocess_to_u8's own kernel takes element counts that are a multiple
    of 8 only (it writes whole 8-element vectors and nothing after the last
    one), so on the shapes with H*W*3 % 8 != 0 its torch reference stands in
    for it; the reference side is checked for every shape."""
    B, H, W = shape
    x = f16_images(B, H, W).cuda()
    got = ops.postprocess_to_i420(x)
    u8_ref = ops.postprocess_to_u8(x.cpu())
    assert torch.equal(got.cpu(), ref_batch(ref_rgb_to_i420, u8_ref))
    assert torch.equal(got, ops.rgb_u8_to_i420(u8_ref.cuda()))
    if x.numel() % 8 == 0:
        u8 = ops.postprocess_to_u8(x)
        assert torch.equal(u8.cpu(), u8_ref)
        assert torch.equal(got, ops.rgb_u8_to_i420(u8))


def test_non_contiguous_inputs_are_made_contiguous():
    big = noise(24, 40, 3)
    view = big[::2, ::2]  # (12, 20, 3)
    assert not view.is_contiguous()
    assert torch.equal(ops.rgb_u8_to_i420(big.cuda()[::2, ::2]).cpu(),
                       ref_rgb_to_i420(view.contiguous()))
    planes = ref_rgb_to_i420(noise(12, 40, 4))  # (18, 40)
    pv = planes[:, ::2]  # (18, 20): an 12x20 picture's worth of bytes
    assert not pv.is_contiguous()
    assert torch.equal(ops.i420_to_rgb_u8(planes.cuda()[:, ::2]).cpu(),
                       ref_i420_to_rgb(pv.contiguous()))
    img = f16_images(1, 12, 40)[0]
    assert torch.equal(ops.postprocess_to_i420(img.cuda()[:, ::2]).cpu(),
                       ref_rgb_to_i420(ops.postprocess_to_u8(img[:, ::2].contiguous())))


@pytest.mark.parametrize("guard", [1, 6, 64])
@pytest.mark.parametrize("shape", [(2, 4, 24), (1, 38, 50), (2, 6, 10)], ids=shape_id)
def test_guard_bytes_untouched(shape, guard):
    """Outputs written into the middle of a larger buffer: nothing outside
    the frames changes, whatever the alignment of the first frame (odd
    offsets take the scalar path)."""
    B, H, W = shape
    x = torch.stack([noise(H, W, 50 + b) for b in range(B)])
    n = B * H * W * 3 // 2

    def guarded(count):
        buf = torch.full((guard + count + guard,), 0xAB, dtype=torch.uint8, device="cuda")
        return buf, buf[guard:guard + count]

    def guards_ok(buf):
        return bool((buf[:guard] == 0xAB).all()) and bool((buf[-guard:] == 0xAB).all())

    buf, mid = guarded(n)
    out = mid.view(B, H * 3 // 2, W)
    ops.rgb_u8_to_i420(x.cuda(), out=out)
    want = ref_batch(ref_rgb_to_i420, x)
    assert torch.equal(out.cpu(), want) and guards_ok(buf)

    buf, mid = guarded(n)
    out = mid.view(B, H * 3 // 2, W)
    img = f16_images(B, H, W)
    ops.postprocess_to_i420(img.cuda(), out=out)
    assert torch.equal(out.cpu(), ref_batch(ref_rgb_to_i420, ops.postprocess_to_u8(img)))
    assert guards_ok(buf)

    buf, mid = guarded(B * H * W * 3)
    out = mid.view(B, H, W, 3)
    # the input at a shifted base as well
    _, src = guarded(n)
    src = src.view(B, H * 3 // 2, W)
    src.copy_(want)
    ops.i420_to_rgb_u8(src, out=out)
    assert torch.equal(out.cpu(), ref_batch(ref_i420_to_rgb, want)) and guards_ok(buf)


def test_error_paths_gpu():
    with pytest.raises(ValueError):
        ops.rgb_u8_to_i420(torch.zeros((5, 4, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.i420_to_rgb_u8(torch.zeros((6, 5), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.i420_to_rgb_u8(torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.postprocess_to_i420(torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.rgb_u8_to_i420(torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"),
                           out=torch.zeros((6, 4), dtype=torch.uint8))  # CPU out


def test_postprocess_to_i420_graph_capture():
    """One linear stream, no parallel branches: capture, then replay on new
    input written into the static buffer."""
    B, H, W = 1, 48, 64
    static_in = f16_images(B, H, W).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.postprocess_to_i420(static_in)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        static_out = ops.postprocess_to_i420(static_in)
    gen = torch.Generator().manual_seed(21)
    new = (torch.rand((B, H, W, 3), generator=gen) * 2.4 - 1.2).to(torch.float16)
    static_in.copy_(new.cuda())
    g.replay()
    torch.cuda.synchronize()
    want = ref_batch(ref_rgb_to_i420, ops.postprocess_to_u8(new))
    assert torch.equal(static_out.cpu(), want)


# ---------------------------------------------------------------------------
# graph engines (SD-Turbo 512x512 1-step, the config of tests/test_fit_gpu.py)
# ---------------------------------------------------------------------------
def _run(e, f):
    out = e(f)
    e.sync_output()
    return out.clone()


@pytest.fixture(scope="module")
def engines_run():
    """Two identically built pipelined graph engines, one returning RGB and
    one I420, fed the same frames in the same order (the order matters only
    in that both see it)."""
    f = noise(512, 512, 77)
    small = noise(360, 640, 78)
    i_f, i_small = ref_rgb_to_i420(f), ref_rgb_to_i420(small)
    res = {}
    for fmt in ("rgb", "i420"):
        cfg = sd_turbo_config(device="cuda", use_hip_graph=True)
        cfg.output_format = fmt
        e = StreamDiffusionEngine(cfg)
        e.prepare()
        r = {"rgb_fed": _run(e, ref_i420_to_rgb(i_f)),
             "i420_fed": _run(e, i_f)}
        r["fmt_same"] = e.stats()["ingest"]
        r["fit_rgb_fed"] = _run(e, ref_i420_to_rgb(i_small))
        r["fit_i420_fed"] = _run(e, i_small)
        r["fmt_fit"] = e.stats()["ingest"]
        res[fmt] = r
    return res


def test_engine_i420_input_equals_rgb_input(engines_run):
    r = engines_run["rgb"]
    assert r["rgb_fed"].shape == (512, 512, 3)
    assert torch.equal(r["i420_fed"], r["rgb_fed"])
    assert r["fmt_same"]["source_format"] == ["i420"]
    assert r["fmt_same"]["last_source_size"] == [[512, 512]]


def test_engine_i420_input_through_fit_path(engines_run):
    r = engines_run["rgb"]
    assert torch.equal(r["fit_i420_fed"], r["fit_rgb_fed"])
    assert not torch.equal(r["fit_i420_fed"], r["i420_fed"])
    assert r["fmt_fit"]["source_format"] == ["i420"]
    assert r["fmt_fit"]["last_source_size"] == [[360, 640]]


def test_engine_i420_output_equals_converted_rgb_output(engines_run):
    rgb, yuv = engines_run["rgb"], engines_run["i420"]
    for k in ("rgb_fed", "i420_fed", "fit_rgb_fed", "fit_i420_fed"):
        assert yuv[k].shape == (768, 512) and yuv[k].dtype == torch.uint8
        assert torch.equal(yuv[k].cpu(), ref_rgb_to_i420(rgb[k].cpu())), k
