"""Op dispatch: hand-written HIP/CDNA4 kernels on GPU, torch reference on CPU.

The GPU activation layout is NHWC throughout (implicit-GEMM friendly on MFMA:
the K = (r,s,c) gather reads 16B-contiguous channel runs — see
ops/csrc/conv2d.hip). The torch reference path permutes to NCHW for
F.conv2d and back; it exists for CPU tests and as the numerics golden that
GPU tests compare the HIP kernels against (SURVEY.md §4 item b).

Replaces (MI355X-natively) reference components N3-N7 of SURVEY.md §2.2:
CV-CUDA convertto/reformat (lib/pipeline.py:61-63) -> fused pre/post kernels;
TensorRT UNet/VAE engines (lib/wrapper.py:409-512) -> these kernels + hipGraph.

Dispatch policy: fp16 tensors on a CUDA/HIP device take the HIP kernels and
RAISE if the extension is missing (no silent eager fallback on GPU). fp32 or
CPU tensors take the torch reference path (that is what GPU numerics tests
compare against).
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

_EXT = None
_EXT_ERR: str | None = None

ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2


def hip_ext():
    """Load the in-tree HIP extension (built by setup.py / __graft_entry__.build)."""
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        from . import _load_ext

        _EXT = _load_ext.load()
    except Exception as e:  # pragma: no cover - exercised only on GPU boxes
        _EXT_ERR = f"{type(e).__name__}: {e}"
        _EXT = None
    return _EXT


def hip_available() -> bool:
    return torch.cuda.is_available() and hip_ext() is not None


def _require_ext():
    ext = hip_ext()
    if ext is None:
        raise RuntimeError(
            "HIP extension not available on a GPU device "
            f"(load error: {_EXT_ERR}). Build it with "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950); "
            "silent eager fallback on GPU is disabled by design."
        )
    return ext


_F16 = (torch.float16,)
_F16_OR_U8 = (torch.float16, torch.uint8)


def _use_hip(x: torch.Tensor, dtypes: tuple | None = _F16) -> bool:
    """The one "runs on the kernel" predicate: x is on the device, of one of
    the dtypes the op's kernel takes (None: the op checks dtypes itself), and
    AIRTC_FORCE_EAGER=1 is not set (read per call)."""
    if not x.is_cuda or (dtypes is not None and x.dtype not in dtypes):
        return False
    return os.environ.get("AIRTC_FORCE_EAGER") != "1"


def uses_hip(x: torch.Tensor) -> bool:
    """Would an op on this tensor run its HIP kernel (rather than the torch
    reference: CPU, non-f16, AIRTC_FORCE_EAGER=1)?"""
    return _use_hip(x)


# ---------------------------------------------------------------------------
# weight caches: tensors derived from a weight, hung on its parameter/module
# ---------------------------------------------------------------------------

# every attribute name weight_cache has ever set; drop_weight_caches removes
# exactly these, so a new cache needs no edit anywhere else
_WEIGHT_CACHE_ATTRS: set = set()


def _same_key(a, b) -> bool:
    """Cache keys: tensors by identity, anything else by value, tuples
    elementwise."""
    if isinstance(a, tuple) and isinstance(b, tuple):
        return len(a) == len(b) and all(map(_same_key, a, b))
    if a is b:
        return True
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return False
    return a == b


def weight_cache(owner, name: str, build, key=None):
    """build() once per owner (a parameter or a module), kept on it as the
    attribute `name` and recorded in the registry. `key` is whatever else
    the value was built from (a second tensor, a scale, a device): another
    key rebuilds. Stored as (key, value)."""
    _WEIGHT_CACHE_ATTRS.add(name)
    c = getattr(owner, name, None)
    if c is None or not _same_key(c[0], key):
        c = (key, build())
        setattr(owner, name, c)
    return c[1]


def weight_cache_names() -> frozenset:
    return frozenset(_WEIGHT_CACHE_ATTRS)


def drop_weight_caches(module: torch.nn.Module) -> None:
    """Remove every weight_cache entry from the module tree and its
    parameters: call after any in-place weight change."""
    for m in module.modules():
        for owner in (m, *m.parameters(recurse=False)):
            for name in _WEIGHT_CACHE_ATTRS:
                if hasattr(owner, name):
                    delattr(owner, name)


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    """The contiguous f32 copy of a bias / gamma / beta the kernels read."""
    return weight_cache(t, name, lambda: t.detach().float().contiguous())


def _gemm_layout(weight: torch.Tensor) -> torch.Tensor:
    """(O,I,R,S) -> the conv kernels' (O, R*S*I) f16 GEMM layout."""
    return weight_cache(
        weight, "_airtc_wperm",
        lambda: weight.detach().permute(0, 2, 3, 1)
        .reshape(weight.shape[0], -1).contiguous().half())


# ---------------------------------------------------------------------------
# torch reference pieces shared by the CPU / eager paths
# ---------------------------------------------------------------------------

def _act_ref(y: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_SILU:
        return F.silu(y)
    if act == ACT_RELU:
        return F.relu(y)
    return y


def _in_affine_ref(x: torch.Tensor, in_affine: torch.Tensor,
                   in_act: int) -> torch.Tensor:
    """f32 act(x * s + t) with the (B, C, 2) per-channel pairs of in_affine."""
    aff = in_affine.float()
    xf = x.float() * aff[:, None, None, :, 0] + aff[:, None, None, :, 1]
    return _act_ref(xf, in_act)


def _epilogue_ref(y, channel_bias, residual, act: int) -> torch.Tensor:
    """The conv epilogue on an f32 NHWC result (bias already added)."""
    if channel_bias is not None:
        y = y + channel_bias.float()[:, None, None, :]
    if residual is not None:
        y = y + residual.float()
    return _act_ref(y, act)


def _e4m3(y: torch.Tensor, scale: float) -> torch.Tensor:
    """float8_e4m3fn codes of y at `scale`, as the kernels encode them:
    multiply by the f32 reciprocal, clamp to +-448, round to nearest even."""
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(
        scale, dtype=torch.float32)
    return (y.float() * inv).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)


def _resize_u8_ref(win: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    """(h, w, 3) u8 -> (oh, ow, 3) u8, antialiased triangle filter in f32,
    round-half-even, clamp; an equal-size window comes back as it is."""
    if tuple(win.shape[:2]) == (oh, ow):
        return win
    x = win.permute(2, 0, 1).unsqueeze(0).to(torch.float32)
    x = F.interpolate(x, size=(oh, ow), mode="bilinear", antialias=True,
                      align_corners=False)
    return x.round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0)


# ---------------------------------------------------------------------------
# conv2d (NHWC activations, OIHW weights)
# ---------------------------------------------------------------------------

def _switch(name: str, default: str = "1") -> bool:
    """A/B switch, read per call: NAME=0 is off, NAME=1 on, unset the
    default."""
    return os.environ.get(name, default) != "0"


def _tiny_pack(weight: torch.Tensor) -> torch.Tensor:
    """(O,I,R,S) -> the tiny-IC kernel's (36, O) f32 pack: row k is column k
    of the (O, R*S*I) GEMM layout, rows past R*S*I zero."""
    O = weight.shape[0]
    w = weight.detach().permute(0, 2, 3, 1).reshape(O, -1).half().float()
    out = torch.zeros((36, O), dtype=torch.float32, device=weight.device)
    out[: w.shape[1]] = w.t()
    return out.contiguous()


def _tail_pack(weight, w_perm, bias, w2, b2):
    """Packed (O, R*S*I + C2) f16 weight and summed f32 bias of a conv with
    a pointwise tail, cached on the conv's weight (`_airtc_wtail`,
    `_airtc_btail`) and keyed on the tensors they were built from."""
    def total_bias():
        parts = [b.detach().float() for b in (bias, b2) if b is not None]
        if not parts:
            return None
        return (parts[0] + parts[1] if len(parts) == 2 else parts[0]).contiguous()

    w_tail = weight_cache(
        weight, "_airtc_wtail",
        lambda: torch.cat([w_perm, _gemm_layout(w2)], dim=1).contiguous(),
        key=w2)
    return w_tail, weight_cache(weight, "_airtc_btail", total_bias,
                                key=(bias, b2))


def conv2d_nhwc(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor | None = None,
    stride: int = 1,
    padding: int = 1,
    fuse_silu: bool = False,
    act: int | None = None,
    residual: torch.Tensor | None = None,
    channel_bias: torch.Tensor | None = None,
    in_affine: torch.Tensor | None = None,
    in_act: int = ACT_NONE,
    stats_groups: int | None = None,
    tail: tuple | None = None,
    upsample2x: bool = False,
    pad_hi: int = 0,
) -> torch.Tensor:
    """x: (B,H,W,C) contiguous; weight: (O,I,R,S) [torch layout]; out (B,H',W',O).

    pad_hi: extra zero rows / columns at the bottom and right only, on top
      of the symmetric `padding` — diffusers' VAE downsample is
      F.pad(x, (0,1,0,1)) then a stride-2 conv with padding 0, i.e.
      padding=0, pad_hi=1. H' = (H + 2*padding + pad_hi - R) // stride + 1.
      GPU: a field of the conv record; the kernels' bounds predicates zero
      the taps, no padded copy.

    tail=(x2, w2, b2): adds the pointwise conv W2·x2 (+ b2) to the result
      before the epilogue — a resnet's 1x1 shortcut. x2 is (B,H',W',C2), w2
      (O,C2,1,1), b2 (O,) or None. GPU: one GEMM over the longer K
      (R*S*C + C2) against a packed weight cached on `weight` — the
      shortcut's conv, its finalize and the f16 rounding of the skip
      disappear. Folded when stride == 1 and C, C2 are multiples of 32;
      otherwise, and with AIRTC_CONV_TAIL=0, the shortcut runs as its own
      conv and comes in as the residual. in_affine applies to x only.
    upsample2x: the conv reads nearest-2x(x) — x is (B,H/2,W/2,C). GPU: a
      shift in the A-load address, bit-identical to upsample_nearest2x_nhwc
      followed by the conv. Opt-in (AIRTC_CONV_UP=1, C % 32 == 0): faster
      per kernel, within noise on the headline frame; otherwise the separate
      upsample kernel runs in front of the conv.

    GPU path: implicit-GEMM on MFMA with on-the-fly im2col gather and inline
    zero-padding (ops/csrc/conv2d.hip). Weights are lazily pre-transformed
    to the (O, R*S*I) GEMM layout and cached on the parameter (the AOT
    `build` step warms every cache before hipGraph capture).

    Epilogue fusion (order): y = act(conv + bias + channel_bias + residual)
      channel_bias: (B, O) — the resnet time-embedding add
      residual:     broadcast-free tensor of the output shape — skip adds
    Input fusion: in_affine (B, C, 2) f32 applies x*s+t (then in_act) to
      every input element AT LOAD TIME — the fused-GroupNorm path
      (group_norm_coeffs); the producing apply kernel and its activation
      round-trip through HBM disappear.
    stats_groups: the group count G of a GroupNorm that consumes THIS
      output directly. On split-K shapes the finalize pass then also emits
      the norm's partial sum/sumsq, and they ride on the returned tensor as
      `_airtc_gn_part` for group_norm_silu_nhwc, whose own stats pass
      disappears. Only a hint, and opt-in (AIRTC_FIN_STATS=1; measured
      neutral end to end): without the switch, on shapes that take no
      finalize pass and on the CPU reference path nothing is attached and
      the norm runs as usual.
    """
    if act is None:
        act = ACT_SILU if fuse_silu else ACT_NONE
    if _use_hip(x):
        ext = _require_ext()
        O, I, R, S = weight.shape
        mfma = I % 32 == 0
        if upsample2x and not (mfma and _switch("AIRTC_CONV_UP", "0")):
            x = upsample_nearest2x_nhwc(x)
            upsample2x = False
        x2 = None
        if tail is not None:
            x2, w2, b2 = tail
            if (mfma and stride == 1 and w2.shape[1] % 32 == 0
                    and tuple(w2.shape[2:]) == (1, 1) and _use_hip(x2)
                    and _switch("AIRTC_CONV_TAIL")):
                x2 = x2.contiguous()
                if upsample2x:  # one addressing mode per kernel launch
                    x = upsample_nearest2x_nhwc(x)
                    upsample2x = False
            else:
                # the pair: the shortcut as its own conv, read back as the
                # residual
                residual = conv2d_nhwc(x2, w2, b2, 1, 0, residual=residual)
                x2 = tail = None
        # 4-/3-channel conv_in layers: lanes-along-OC kernel (conv2d.hip,
        # conv2d_tinyic_kernel), at any size — at 512²x3->64 it measured
        # 49.3 us against 55.1 us for the pad-to-32 route below (zeros +
        # copy_ + MFMA conv). AIRTC_CONV_TINYIC=0 restores the per-pixel
        # kernel / the pad route.
        if (I <= 4 and R * S * I <= 36 and in_affine is None
                and _switch("AIRTC_CONV_TINYIC")):
            return ext.conv2d_tinyic(
                x=x,
                w_tiny=weight_cache(weight, "_airtc_wtiny",
                                    lambda: _tiny_pack(weight)),
                bias=None if bias is None else _f32(bias, "_airtc_b32"),
                cbias=None if channel_bias is None else channel_bias.contiguous(),
                residual=None if residual is None else residual.contiguous(),
                R=R, S=S, stride=stride, pad=padding, act=act, pad_hi=pad_hi)
        # Other small-IC convs at large spatial (and the 3/4-channel conv_in
        # layers with AIRTC_CONV_TINYIC=0) measured 129us at 512² on the
        # scalar small-IC kernel; zero-padding
        # the input channels to 32 routes them through the MFMA path
        # (numerics identical: zero channels contribute nothing). The pad
        # copy is a ~1.5 MB -> 16 MB expansion, trivial against HBM3E.
        if I < 32 and in_affine is None and x.shape[1] * x.shape[2] >= 16384:
            xp = torch.zeros((*x.shape[:3], 32), dtype=x.dtype, device=x.device)
            xp[..., :I].copy_(x)
            w_pad = weight_cache(
                weight,
                "_airtc_wpad32",
                lambda: torch.cat(
                    [weight.detach(),
                     torch.zeros((O, 32 - I, R, S), dtype=weight.dtype,
                                 device=weight.device)], dim=1).contiguous(),
            )
            return conv2d_nhwc(xp, w_pad, bias, stride, padding, fuse_silu,
                               act=act, residual=residual,
                               channel_bias=channel_bias,
                               stats_groups=stats_groups, pad_hi=pad_hi)
        w_perm = _gemm_layout(weight)
        b32 = None if bias is None else _f32(bias, "_airtc_b32")
        if x2 is not None:
            # one (O, R*S*I + C2) weight and one summed f32 bias per conv
            # weight, rebuilt if another shortcut is passed with it
            w_perm, b32 = _tail_pack(weight, w_perm, bias, tail[1], tail[2])
        want_stats = bool(stats_groups) and act == ACT_NONE
        y, part = ext.conv2d(
            x=x, w_perm=w_perm, bias=b32,
            cbias=None if channel_bias is None else channel_bias.contiguous(),
            residual=None if residual is None else residual.contiguous(),
            R=R, S=S, stride=stride, pad=padding, act=act,
            in_affine=None if in_affine is None else in_affine.contiguous(),
            in_act=in_act, stats_groups=stats_groups if want_stats else 0,
            x2=x2, upsample2x=upsample2x, pad_hi=pad_hi)
        if part is not None:
            # (partials, G, version): the norm ignores them if the tensor
            # was written in place after the conv
            y._airtc_gn_part = (part, stats_groups, y._version)
        return y

    if in_affine is not None:
        x = _in_affine_ref(x, in_affine, in_act).to(x.dtype)
    xc = x.permute(0, 3, 1, 2)
    if upsample2x:
        xc = F.interpolate(xc, scale_factor=2, mode="nearest")
    if pad_hi:
        if pad_hi < 0:
            raise ValueError(f"pad_hi must be >= 0, got {pad_hi}")
        xc = F.pad(xc, (0, pad_hi, 0, pad_hi))
    y = F.conv2d(xc.float(), weight.float(), None if bias is None else bias.float(),
                 stride=stride, padding=padding)
    if tail is not None:
        x2, w2, b2 = tail
        y = y + F.conv2d(x2.permute(0, 3, 1, 2).float(), w2.float(),
                         None if b2 is None else b2.float())
    y = _epilogue_ref(y.permute(0, 2, 3, 1), channel_bias, residual, act)
    return y.to(x.dtype).contiguous()


# ---------------------------------------------------------------------------
# fp8 (OCP e4m3) conv — the MX-scaled MFMA serving tier
# ---------------------------------------------------------------------------

FP8_MAX = 448.0  # largest finite e4m3fn magnitude


def quantize_weight_fp8(weight: torch.Tensor):
    """(O,I,R,S) f16/f32 -> (uint8 (O, R*S*I) e4m3 codes, f32 (O,) scales).

    Per-out-channel symmetric absmax scaling; codes are w/scale rounded RNE
    (torch's e4m3fn cast is bit-identical to the gfx950 v_cvt encode at
    scale 1 — verified by tools/fp8_probe.py). K order matches the f16
    kernel's (r, s, ic) GEMM layout."""
    O = weight.shape[0]
    w = weight.detach().float().permute(0, 2, 3, 1).reshape(O, -1)
    scale = (w.abs().amax(dim=1) / FP8_MAX).clamp_min(1e-12)
    q = (w / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), scale.contiguous()


def fp8_roundtrip(x: torch.Tensor, scale: float) -> torch.Tensor:
    """Emulate the kernel's activation quantization:
    e4m3(clamp(x * (1/scale), +-448)) * scale — the kernel multiplies by the
    f32 reciprocal (v_cvt_pk_fp8_f32 path), so the emulation does too.
    Reference for tests and the CPU path (f32 in/out)."""
    return _e4m3(x, scale).to(torch.float32) * scale


def conv2d_fp8_nhwc(
    x: torch.Tensor,
    weight: torch.Tensor,
    a_scale: float,
    bias: torch.Tensor | None = None,
    stride: int = 1,
    padding: int = 1,
    act: int = ACT_NONE,
    residual: torch.Tensor | None = None,
    channel_bias: torch.Tensor | None = None,
    in_affine: torch.Tensor | None = None,
    in_act: int = ACT_NONE,
    out_fp8_scale: float | None = None,
) -> torch.Tensor:
    """fp8 serving-tier conv: same contract as conv2d_nhwc plus a_scale (the
    calibrated per-tensor activation scale). GPU: conv2d_fp8.hip — weights
    pre-quantized per-OC (cached on the parameter), activations quantized in
    the staging loads AFTER the fused affine/activation. CPU/eager: exact
    emulation of the same quantization math (the GPU numerics golden).

    x may be f16 (the kernel quantizes in its staging loads) or u8 e4m3
    codes already scaled by a_scale (producer-quantized, e.g. the output of
    group_norm_silu_nhwc(fp8_scale=...)) — the fast path.

    out_fp8_scale: ask the epilogue to emit e4m3 codes at that scale
    (chained fp8 layers, e.g. TAESD conv stacks). The GPU honours it only
    on split-K-free shapes — dispatch on the RETURNED dtype.

    Requires IC % 64 == 0 (use conv2d_nhwc for other layers)."""
    O, I, R, S = weight.shape
    x_q8 = x.dtype == torch.uint8
    if _use_hip(x, _F16_OR_U8):
        ext = _require_ext()
        w_fp8, w_scale = weight_cache(weight, "_airtc_wfp8",
                                      lambda: quantize_weight_fp8(weight))
        dq = weight_cache(weight, "_airtc_wdq",
                          lambda: (w_scale * a_scale).contiguous(), key=a_scale)
        return ext.conv2d_fp8(
            x=x, w_fp8=w_fp8, dq=dq, a_scale=a_scale,
            bias=None if bias is None else _f32(bias, "_airtc_b32"),
            cbias=None if channel_bias is None else channel_bias.contiguous(),
            residual=None if residual is None else residual.contiguous(),
            R=R, S=S, stride=stride, pad=padding, act=act,
            in_affine=None if in_affine is None else in_affine.contiguous(),
            in_act=in_act,
            out_scale=0.0 if out_fp8_scale is None else out_fp8_scale)

    # emulation path (CPU tests + GPU numerics golden): quantize exactly as
    # the kernel does, then run the f32 reference conv
    if x_q8:
        assert in_affine is None, "pre-quantized input excludes input affine"
        xq = x.view(torch.float8_e4m3fn).to(torch.float32) * a_scale
    else:
        xf = x.float() if in_affine is None \
            else _in_affine_ref(x, in_affine, in_act)
        xq = fp8_roundtrip(xf, a_scale)
    w_fp8, w_scale = quantize_weight_fp8(weight)
    wdec = w_fp8.view(torch.float8_e4m3fn).to(torch.float32) * w_scale[:, None]
    wdec = wdec.reshape(O, R, S, I).permute(0, 3, 1, 2)
    y = F.conv2d(xq.permute(0, 3, 1, 2), wdec,
                 None if bias is None else bias.float(),
                 stride=stride, padding=padding).permute(0, 2, 3, 1)
    y = _epilogue_ref(y, channel_bias, residual, act)
    if out_fp8_scale is not None:
        return _e4m3(y, out_fp8_scale).view(torch.uint8).contiguous()
    # u8 input carries no output dtype — use the model (weight) dtype
    return y.to(weight.dtype if x_q8 else x.dtype).contiguous()


# ---------------------------------------------------------------------------
# normalisations
# ---------------------------------------------------------------------------

def group_norm_coeffs(
    x: torch.Tensor,
    num_groups: int,
    gamma: torch.Tensor,
    beta: torch.Tensor,
    eps: float = 1e-5,
) -> torch.Tensor:
    """Per-(batch, channel) affine pairs (B, C, 2) f32 such that
    gn(x)[..., c] == x[..., c] * s + t — the input-side half of the fused
    GN->conv (conv2d_nhwc in_affine). GPU: stats kernel + a tiny coeffs
    kernel; the full-tensor apply pass disappears."""
    if _use_hip(x):
        if (x.shape[-1] // num_groups) % 2 != 0:
            raise ValueError("group_norm kernel needs even channels-per-group")
        return _require_ext().group_norm_coeffs(
            x, num_groups, _f32(gamma, "_airtc_g32"), _f32(beta, "_airtc_b32"),
            eps)
    b, c = x.shape[0], x.shape[-1]
    xf = x.reshape(b, -1, num_groups, c // num_groups).permute(0, 2, 1, 3).float()
    mean = xf.mean(dim=(2, 3))                             # (B, G)
    rstd = (xf.var(dim=(2, 3), unbiased=False) + eps).rsqrt()
    mean_c = mean.repeat_interleave(c // num_groups, dim=1)
    rstd_c = rstd.repeat_interleave(c // num_groups, dim=1)
    s = gamma.float()[None] * rstd_c
    t = beta.float()[None] - mean_c * s
    return torch.stack([s, t], dim=-1).contiguous()


def group_norm_silu_nhwc(
    x: torch.Tensor,
    num_groups: int,
    gamma: torch.Tensor,
    beta: torch.Tensor,
    eps: float = 1e-5,
    silu: bool = True,
    fp8_scale: float | None = None,
) -> torch.Tensor:
    """Fused GroupNorm(+SiLU) on NHWC. GPU: single kernel, wave-reduced stats.

    fp8_scale: when set, the apply pass QUANTIZES its output to e4m3 codes
    (u8 tensor, q = clamp(act(gn(x))/fp8_scale, +-448)) for the fp8 conv's
    pre-quantized input path — producer-side quantization: one encode per
    element instead of one per 3x3 tap, and half the GN output traffic."""
    if _use_hip(x):
        if (x.shape[-1] // num_groups) % 2 != 0:
            raise ValueError(
                f"group_norm kernel needs even channels-per-group, got "
                f"C={x.shape[-1]} groups={num_groups}"
            )
        ext = _require_ext()
        g32, b32 = _f32(gamma, "_airtc_g32"), _f32(beta, "_airtc_b32")
        act = ACT_SILU if silu else ACT_NONE
        # partial statistics the producing conv's finalize left on x
        # (conv2d_nhwc stats_groups): same tensor, same G, unmodified since
        part = None
        tag = getattr(x, "_airtc_gn_part", None)
        if tag is not None and tag[1] == num_groups and tag[2] == x._version:
            part = tag[0]
        if fp8_scale is not None:
            return ext.group_norm_silu_fp8(x, num_groups, g32, b32, eps, act,
                                           fp8_scale, part)
        return ext.group_norm_silu(x, num_groups, g32, b32, eps, act, part)
    b, h, w, c = x.shape
    xc = x.permute(0, 3, 1, 2).float()
    y = F.group_norm(xc, num_groups, gamma.float(), beta.float(), eps)
    y = y.permute(0, 2, 3, 1)
    if silu:
        y = F.silu(y)
    if fp8_scale is not None:
        return _e4m3(y, fp8_scale).view(torch.uint8).contiguous()
    return y.to(x.dtype).contiguous()


def layer_norm(
    x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5
) -> torch.Tensor:
    # the kernel reads 8 channels per lane; other widths take the torch path
    if _use_hip(x) and x.shape[-1] % 8 == 0:
        return _require_ext().layer_norm(
            x, _f32(gamma, "_airtc_g32"), _f32(beta, "_airtc_b32"), eps)
    return F.layer_norm(x.float(), (x.shape[-1],), gamma.float(), beta.float(), eps).to(x.dtype)


# ---------------------------------------------------------------------------
# attention / MLP
# ---------------------------------------------------------------------------

_ATTN_DIMS = (32, 64, 96, 128, 160)
# one wide head (ops/csrc/attention_wide.hip): served as it is, never a
# padding target
_ATTN_WIDE_DIMS = (512,)


def attention_serves(head_dim: int) -> bool:
    """Does a HIP attention kernel take this head width (zero-padded to the
    next template size where needed)?"""
    return 0 < head_dim <= max(_ATTN_DIMS) or head_dim in _ATTN_WIDE_DIMS


def attention(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int,
    scale: float | None = None,
) -> torch.Tensor:
    """q: (B, Lq, C); k,v: (B, Lk, C). Returns (B, Lq, C).

    GPU: flash-style fused kernel (online softmax, MFMA QK^T and PV,
    LDS-tiled K/V) — ops/csrc/attention.hip; head_dim 512 (the KL VAE's one
    wide head) runs ops/csrc/attention_wide.hip. head_dim % 32 == 0 runs
    zero-copy on (b,h)-strided views; other head dims are zero-padded to
    the next supported size (softmax-invariant — but pass the TRUE-dim
    scale when the inputs were padded upstream).
    """
    if _use_hip(q):
        ext = _require_ext()
        b, lq, c = q.shape
        lk = k.shape[1]
        d = c // num_heads
        if scale is None:
            scale = 1.0 / math.sqrt(d)
        if d in _ATTN_DIMS or d in _ATTN_WIDE_DIMS:
            return ext.attention_bhlc(q, k, v, num_heads, scale)
        if d > max(_ATTN_DIMS):
            raise ValueError(
                f"attention: head_dim {d} has no kernel; supported are up to "
                f"{max(_ATTN_DIMS)} (padded to one of {_ATTN_DIMS}) and "
                f"{_ATTN_WIDE_DIMS}")
        dpad = min(x for x in _ATTN_DIMS if x >= d)

        def rearrange(t, L):
            th = t.reshape(b, L, num_heads, d)
            th = F.pad(th, (0, dpad - d))
            return th.permute(0, 2, 1, 3).reshape(b * num_heads, L, dpad).contiguous()

        o = ext.attention_bhlc(rearrange(q, lq), rearrange(k, lk), rearrange(v, lk), 1, scale)
        o = o.view(b, num_heads, lq, dpad)[..., :d]
        return o.permute(0, 2, 1, 3).reshape(b, lq, c).contiguous()

    b, lq, c = q.shape
    d = c // num_heads
    qh = q.reshape(b, lq, num_heads, d).permute(0, 2, 1, 3).float()
    kh = k.reshape(b, -1, num_heads, d).permute(0, 2, 1, 3).float()
    vh = v.reshape(b, -1, num_heads, d).permute(0, 2, 1, 3).float()
    o = F.scaled_dot_product_attention(qh, kh, vh, scale=scale)
    return o.permute(0, 2, 1, 3).reshape(b, lq, c).to(q.dtype)


def linear(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor | None = None,
    residual: torch.Tensor | None = None,
) -> torch.Tensor:
    """Linear projection on hipBLASLt (allowed: library GEMMs).

    Projections that carry a residual add (attention out-proj, FF out,
    transformer proj_out) run as ONE library call on the GPU: the bias
    rides in the GEMM's bias epilogue and the residual is its C operand
    with beta = 1 (ops/csrc/gemm_lt.cpp), so the separate aten add and its
    second f16 rounding disappear. x, weight, bias and residual must be
    contiguous f16 there; a strided one raises, it is not copied.
    AIRTC_LT_EPILOGUE=0 restores F.linear + add.
    AIRTC_FUSED_PROJ=1 runs these projections through OUR MFMA kernel as a
    1x1 conv with the residual fused into its epilogue instead."""
    # Measured on MI355X: hipBLASLt + the trailing aten add beats this fused
    # path at SD shapes (118 -> 109 fps when enabled); keep it opt-in until
    # the MFMA GEMM closes the gap (AIRTC_FUSED_PROJ=1).
    if residual is not None and os.environ.get("AIRTC_FUSED_PROJ") == "1" \
            and _use_hip(x) and x.dim() == 3 and weight.shape[1] % 32 == 0:
        ext = _require_ext()
        b, l, c = x.shape
        w16 = weight_cache(weight, "_airtc_w16",
                           lambda: weight.detach().contiguous().half())
        y, _ = ext.conv2d(
            x=x.reshape(b, l, 1, c), w_perm=w16,
            bias=None if bias is None else _f32(bias, "_airtc_b32"),
            residual=residual.reshape(b, l, 1, -1).contiguous(), R=1, S=1)
        return y.reshape(b, l, -1)
    if residual is not None and _use_hip(x) \
            and os.environ.get("AIRTC_LT_EPILOGUE") != "0":
        y = _linear_residual_lt(x, weight, bias, residual)
        if y is not None:
            return y
    y = F.linear(x, weight, bias)
    if residual is not None:
        y = y + residual
    return y


# (M, N, K, has_bias) problems that stay on F.linear + add: those measured
# slower as one call than as two (tools/kernel_bench.py "linear + residual",
# profiles/optimization_ladder.md) ...
_LT_UNFUSED_SHAPES: frozenset = frozenset()
# ... and those hipBLASLt offered no algorithm for when first met
_LT_NO_ALGO: set = set()
_LT_SEEN: set = set()


def _linear_residual_lt(x, weight, bias, residual):
    """x·Wᵀ + bias + residual as one hipBLASLt call, or None where the
    problem belongs on the two-kernel path. The path is picked up front by
    shape and dtype; anything the native call rejects after that raises."""
    fn = getattr(_require_ext(), "linear_residual", None)
    if fn is None or weight.dtype != torch.float16 \
            or residual.dtype != torch.float16 \
            or (bias is not None and bias.dtype != torch.float16):
        return None
    n, k = weight.shape
    key = (x.numel() // k, n, k, bias is not None)
    if key in _LT_UNFUSED_SHAPES or key in _LT_NO_ALGO:
        return None
    if key in _LT_SEEN:
        return fn(x, weight, bias, residual)
    try:
        y = fn(x, weight, bias, residual)
    except RuntimeError as e:
        # only "the library has no algorithm for this problem", only on the
        # first call for a shape and never inside a graph capture, where the
        # two paths would bake different kernels into the graph unnoticed
        if _require_ext().LT_NO_ALGORITHM not in str(e) \
                or torch.cuda.is_current_stream_capturing():
            raise
        _LT_NO_ALGO.add(key)
        return None
    _LT_SEEN.add(key)
    return y


def geglu(x: torch.Tensor) -> torch.Tensor:
    """GEGLU activation: split last dim, a * gelu(b). GPU: fused kernel."""
    if _use_hip(x) and x.shape[-1] % 16 == 0:  # inner % 8: 16 B per lane
        return _require_ext().geglu(x)
    a, b = x.chunk(2, dim=-1)
    return (a.float() * F.gelu(b.float())).to(x.dtype)


def silu(x: torch.Tensor) -> torch.Tensor:
    if _use_hip(x) and x.numel() % 8 == 0:
        return _require_ext().silu(x)
    return F.silu(x.float()).to(x.dtype)


def add_act(a: torch.Tensor, b: torch.Tensor, act: int = ACT_NONE) -> torch.Tensor:
    """Fused residual add + optional activation (TAESD add+relu, resnet skips)."""
    if _use_hip(a) and a.numel() % 8 == 0:
        return _require_ext().add_act(a, b, act)
    return _act_ref(a.float() + b.float(), act).to(a.dtype)


# ---------------------------------------------------------------------------
# resampling
# ---------------------------------------------------------------------------

def sched_add_noise(x0: torch.Tensor, noise: torch.Tensor, a32: torch.Tensor,
                    b32: torch.Tensor) -> torch.Tensor:
    """Fused q(x_t|x0): a*x0 + b*noise with per-batch-row f32 coeffs (B,).
    Replaces ~3 aten broadcast kernels in the per-frame hot loop."""
    if _use_hip(x0):
        ext = _require_ext()
        return ext.sched_add_noise(x0, noise, a32.contiguous(), b32.contiguous())
    a = a32.to(x0.dtype).view(-1, *([1] * (x0.dim() - 1)))
    b = b32.to(x0.dtype).view(-1, *([1] * (x0.dim() - 1)))
    return a * x0 + b * noise


def sched_blend(x_t: torch.Tensor, eps: torch.Tensor, a32: torch.Tensor,
                b32: torch.Tensor, c_out32: torch.Tensor,
                c_skip32: torch.Tensor) -> torch.Tensor:
    """Fused LCM denoise step: c_out*(x_t - b*eps)/a + c_skip*x_t.
    Replaces ~5 aten kernels per frame."""
    if _use_hip(x_t):
        ext = _require_ext()
        return ext.sched_blend(x_t.contiguous(), eps.contiguous(),
                               a32.contiguous(), b32.contiguous(),
                               c_out32.contiguous(), c_skip32.contiguous())
    sh = (-1, *([1] * (x_t.dim() - 1)))
    a = a32.view(sh).to(torch.float32)
    b = b32.view(sh).to(torch.float32)
    x0 = (x_t.float() - b * eps.float()) / a
    y = c_out32.view(sh) * x0 + c_skip32.view(sh) * x_t.float()
    return y.to(x_t.dtype)


RCFG_MODES = ("self", "initialize", "full")


def _rcfg_chain(mode: str, eps: torch.Tensor, stock, fbs: int, gm1: float,
                delta: float, g: float) -> torch.Tensor:
    """The torch chain of ResidualCFG's scalar path, stock shift included."""
    if mode == "full":
        half = eps.shape[0] // 2
        eps_u, eps_c = eps[:half], eps[half:]
        return eps_u + g * (eps_c - eps_u)
    eps_c = eps
    if mode == "initialize":
        seed, eps_c = eps[:fbs], eps[fbs:]
        stock[:fbs].copy_(seed)
    out = eps_c + gm1 * (eps_c - delta * stock)
    stock.copy_(torch.cat([eps_c[:fbs], eps_c[:-fbs]], dim=0))
    return out


def rcfg_apply(mode: str, eps: torch.Tensor, fbs: int, *,
               gm1: torch.Tensor | None = None,
               delta: torch.Tensor | None = None,
               stock: torch.Tensor | None = None,
               g: torch.Tensor | None = None) -> torch.Tensor:
    """Residual-CFG step with per-row f32 coefficients (B,), B = output rows.

    self:       out[r] = eps[r] + gm1[r]*(eps[r] - delta[r]*stock[r]), and
                `stock` shifts in place: rows < fbs take eps[r], the others
                eps[r - fbs]
    initialize: eps = [seed(fbs) | cond(B)]; as self on the cond rows, rows
                < fbs read seed[r] where self reads stock[r]
    full:       eps = [uncond(B) | cond(B)]; out[r] = uncond[r] +
                g[r]*(cond[r] - uncond[r]); no stock

    On the GPU this is one HIP launch (f16) that rounds after every
    arithmetic step, bit-identical to the f16 torch chain. Elsewhere it IS
    that chain: whole-batch when the coefficients are uniform, row by row
    when they differ."""
    if mode not in RCFG_MODES:
        raise ValueError(f"mode must be one of {RCFG_MODES}, got {mode!r}")
    full = mode == "full"
    coef = g if full else gm1
    if coef is None or (not full and (delta is None or stock is None)):
        raise ValueError(
            "rcfg_apply: full needs g; self/initialize need gm1, delta, stock")
    if _use_hip(eps):
        ext = _require_ext()
        return ext.rcfg_apply(RCFG_MODES.index(mode), eps.contiguous(), coef,
                              None if full else delta,
                              None if full else stock, fbs)
    B = coef.numel()
    if eps.is_cuda:
        # eager on the device (f32 engine, AIRTC_FORCE_EAGER=1): reading the
        # coefficients back would sync and cannot be captured. Broadcast
        # them instead, f32 math with a rounding to eps.dtype per step —
        # the kernel's arithmetic, op for op.
        sh = (-1, *([1] * (eps.dim() - 1)))
        dt = eps.dtype
        c32 = coef.view(sh)
        if full:
            eps_u, eps_c = eps[:B].float(), eps[B:].float()
            df = (eps_c - eps_u).to(dt).float()
            return (eps_u + (c32 * df).to(dt).float()).to(dt)
        eps_c = eps[eps.shape[0] - B:]
        if mode == "initialize":
            stock[:fbs].copy_(eps[:fbs])
        e = eps_c.float()
        df = (e - (delta.view(sh) * stock.float()).to(dt).float()).to(dt).float()
        out = (e + (c32 * df).to(dt).float()).to(dt)
        stock.copy_(torch.cat([eps_c[:fbs], eps_c[:-fbs]], dim=0))
        return out
    cl = coef.tolist()
    dl = [0.0] * B if full else delta.tolist()
    if all(c == cl[0] for c in cl) and all(d == dl[0] for d in dl):
        return _rcfg_chain(mode, eps, stock, fbs, cl[0], dl[0], cl[0])
    extra = eps.shape[0] - B  # seed rows (initialize) / uncond rows (full)
    out = torch.empty((B, *eps.shape[1:]), dtype=eps.dtype, device=eps.device)
    new_stock = None if full else torch.empty_like(stock)
    for r in range(B):
        if full:
            out[r] = _rcfg_chain(mode, eps[r::B], None, 1, 0.0, 0.0, cl[r])[0]
            continue
        # one-row chain: row r's "stock" is the seed for the first fbs rows
        # of initialize; its shifted stock is filled in below
        s = eps[r] if (mode == "initialize" and r < fbs) else stock[r]
        e = eps[extra + r]
        out[r] = e + cl[r] * (e - dl[r] * s)
        new_stock[r] = e if r < fbs else eps[extra + r - fbs]
    if not full:
        stock.copy_(new_stock)
    return out


def upsample_nearest2x_nhwc(x: torch.Tensor) -> torch.Tensor:
    if _use_hip(x) and x.shape[-1] % 8 == 0:
        return _require_ext().upsample2x(x)
    xc = x.permute(0, 3, 1, 2)
    y = F.interpolate(xc, scale_factor=2, mode="nearest")
    return y.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------
# frame pre/post-processing (replaces CV-CUDA convertto+reformat, N3+N4)
# ---------------------------------------------------------------------------

def preprocess_from_u8(frame_u8: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """u8 (H,W,3) or (B,H,W,3) RGB -> dtype (B,H,W,3) in [-1, 1].

    Fuses the reference's cvcuda.convertto (u8->f32 x 1/255,
    lib/pipeline.py:61) + normalisation; layout stays NHWC (the GPU path
    never needs the reference's NHWC->NCHW reformat, lib/pipeline.py:63).
    """
    if frame_u8.dim() == 3:
        frame_u8 = frame_u8.unsqueeze(0)
    if dtype == torch.float16 and _use_hip(frame_u8, None) \
            and hip_ext() is not None:
        return _require_ext().preprocess_u8(frame_u8.contiguous())
    return (frame_u8.to(torch.float32) / 127.5 - 1.0).to(dtype)


FIT_MODES = ("cover", "contain", "stretch")


def _round_div(a: int, b: int, c: int) -> int:
    """round(a*b/c) in integers, clamped to >= 1."""
    return max(1, (a * b + c // 2) // c)


def fit_geometry(Hs: int, Ws: int, H: int, W: int, mode: str = "cover"):
    """Integer fit geometry for a (Hs, Ws) source into a (H, W) destination.

    Returns ((y0, x0, ch, cw), (oy, ox, oh, ow)): the source window that is
    read and the destination window it is resized into.
      cover   — largest centred source window with the destination's aspect
                ratio; fills the whole destination (edges are cropped)
      contain — whole source into the largest centred destination rectangle
                with the source's aspect ratio (the rest is black bars)
      stretch — whole source into whole destination (aspect not kept)
    """
    if min(Hs, Ws, H, W) < 1:
        raise ValueError(f"empty frame: {(Hs, Ws)} -> {(H, W)}")
    if mode == "cover":
        if Ws * H > Hs * W:
            ch, cw = Hs, min(Ws, _round_div(Hs, W, H))
        else:
            ch, cw = min(Hs, _round_div(Ws, H, W)), Ws
        return ((Hs - ch) // 2, (Ws - cw) // 2, ch, cw), (0, 0, H, W)
    if mode == "contain":
        if Ws * H > Hs * W:
            oh, ow = min(H, _round_div(W, Hs, Ws)), W
        else:
            oh, ow = H, min(W, _round_div(H, Ws, Hs))
        return (0, 0, Hs, Ws), ((H - oh) // 2, (W - ow) // 2, oh, ow)
    if mode == "stretch":
        return (0, 0, Hs, Ws), (0, 0, H, W)
    raise ValueError(f"fit mode must be one of {FIT_MODES}, got {mode!r}")


def fit_frame_u8(src: torch.Tensor, out: torch.Tensor, slot: int,
                 mode: str = "cover") -> None:
    """Fit a u8 RGB frame of ANY size into one slot of a frame buffer.

    src: (Hs, Ws, 3) u8; out: (B, H, W, 3) u8 contiguous, same device. Only
    out[slot] is written: the fitted picture inside the destination window
    of fit_geometry(), zeros outside it. "Crop the source window, then
    resize it" with the separable antialiased triangle filter
    (F.interpolate(mode="bilinear", antialias=True, align_corners=False)),
    f32 accumulation, round-half-even, clamp to [0, 255]; equal-size
    windows are an exact copy.

    GPU: ONE launch of fit_resize_u8 (ops/csrc/elementwise.hip) on the
    current stream, writing straight into the slot. Its tap loops and LDS
    row chunks are sized from the scale at run time, so every downscale
    factor runs on the kernel — nothing is routed to torch on the GPU and
    no tap is ever truncated. CPU tensors and AIRTC_FORCE_EAGER=1 take the
    torch reference below.
    """
    if src.dtype != torch.uint8 or out.dtype != torch.uint8:
        raise TypeError("fit_frame_u8 takes uint8 tensors")
    if src.dim() != 3 or src.shape[-1] != 3 or out.dim() != 4 or out.shape[-1] != 3:
        raise ValueError(
            f"fit_frame_u8 needs src (Hs,Ws,3) and out (B,H,W,3), got "
            f"{tuple(src.shape)} and {tuple(out.shape)}")
    if src.device != out.device:
        raise ValueError(f"src on {src.device} but out on {out.device}")
    if not 0 <= slot < out.shape[0]:
        raise IndexError(f"slot {slot} out of range for {out.shape[0]} slots")
    H, W = out.shape[1], out.shape[2]
    (y0, x0, ch, cw), (oy, ox, oh, ow) = fit_geometry(
        src.shape[0], src.shape[1], H, W, mode)
    if _use_hip(src, None):
        if not out.is_contiguous():
            raise ValueError("out must be contiguous (it is written in place)")
        _require_ext().fit_resize_u8(src.contiguous(), out, slot, y0, x0, ch,
                                     cw, oy, ox, oh, ow)
        return
    win = _resize_u8_ref(src[y0:y0 + ch, x0:x0 + cw], oh, ow)
    dst = out[slot]
    if (oh, ow) != (H, W):
        dst.zero_()
    dst[oy:oy + oh, ox:ox + ow].copy_(win)


def postprocess_to_u8(img: torch.Tensor) -> torch.Tensor:
    """dtype (B,H,W,3) in [-1,1] -> u8 (B,H,W,3). Reference lib/pipeline.py:72-74."""
    if _use_hip(img):
        return _require_ext().postprocess_u8(img.contiguous())
    x = (img.float() + 1.0) * 127.5
    return x.round().clamp(0, 255).to(torch.uint8)


# ---------------------------------------------------------------------------
# edge hint for ControlNet (ops/csrc/canny.hip)
# ---------------------------------------------------------------------------
# The operator, stated once; the HIP kernel and the torch path below are the
# same integer arithmetic and agree bit for bit:
#   Y  = (77R + 150G + 29B + 128) >> 8
#   S  = (5x5 binomial [1,4,6,4,1]^2 of Y, taps clamped to the image, + 128) >> 8
#   gx = (S[y-1,x+1] + 2S[y,x+1] + S[y+1,x+1]) - (S[y-1,x-1] + 2S[y,x-1] + S[y+1,x-1])
#   gy = (S[y+1,x-1] + 2S[y+1,x] + S[y+1,x+1]) - (S[y-1,x-1] + 2S[y-1,x] + S[y-1,x+1])
#        (taps clamped to the image);  M = |gx| + |gy| <= 2040
#   non-maximum suppression in OpenCV's integer sectors, M outside the image
#   counting as 0: ax = |gx|, ay = |gy| << 15, t22 = 13573 ax,
#   t67 = t22 + (ax << 16);
#     ay < t22: keep = M > M[y,x-1] and M >= M[y,x+1]
#     ay > t67: keep = M > M[y-1,x] and M >= M[y+1,x]
#     else, s = -1 if (gx ^ gy) < 0 else 1:
#               keep = M > M[y-1,x-s] and M > M[y+1,x+s]
#   cand = keep and M > low;  strong = keep and M > high
#   E0 = strong;  `reach` times: E <- cand and (3x3 dilation of E)
# The last step is where this differs from cv2.Canny, whose hysteresis
# floods without bound: here a weak edge survives only within `reach` 3x3
# steps of a strong pixel. That makes every pixel a function of the pixels
# within Chebyshev distance reach + 4, which is what lets one kernel launch
# with a fixed shape compute it inside a captured graph.

CANNY_MAX_M = 2040
CANNY_MAX_REACH = 32


def check_canny_thresholds(low, high) -> tuple:
    """(low, high) as ints, 0 <= low <= high <= 2040, else ValueError."""
    try:
        lo, hi = int(low), int(high)
        ok = lo == low and hi == high
    except (TypeError, ValueError) as e:
        raise ValueError(f"canny thresholds must be integers: {e}") from e
    if not ok or isinstance(low, bool) or isinstance(high, bool):
        raise ValueError(f"canny thresholds must be integers, got {low!r}, {high!r}")
    if not 0 <= lo <= hi <= CANNY_MAX_M:
        raise ValueError(
            f"canny thresholds need 0 <= low <= high <= {CANNY_MAX_M}, "
            f"got low={lo}, high={hi}")
    return lo, hi


def _taps(p: torch.Tensor, dy: int, dx: int, replicate: bool) -> torch.Tensor:
    """p[..., y+dy, x+dx] over the whole (B,H,W) plane: coordinates clamped
    to the image (replicate) or zero outside it."""
    H, W = p.shape[-2], p.shape[-1]
    if replicate:
        iy = (torch.arange(H, device=p.device) + dy).clamp_(0, H - 1)
        ix = (torch.arange(W, device=p.device) + dx).clamp_(0, W - 1)
        return p[:, iy][:, :, ix]
    q = F.pad(p, (1, 1, 1, 1))
    return q[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def canny_hint_reference(frames_u8: torch.Tensor, thr: torch.Tensor,
                         reach: int) -> torch.Tensor:
    """The operator above in torch integer arithmetic: (B,H,W,3) u8 and
    (B,2) int (low, high) -> (B,H,W) bool edge map."""
    p = frames_u8.to(torch.int32)
    sh = torch.bitwise_right_shift
    Y = sh(77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128, 8)
    k = (1, 4, 6, 4, 1)
    acc = torch.zeros_like(Y)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            acc += k[dy + 2] * k[dx + 2] * _taps(Y, dy, dx, True)
    S = sh(acc + 128, 8)

    def s(dy, dx):
        return _taps(S, dy, dx, True)

    gx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    gy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    ax, ay = gx.abs(), gy.abs() << 15
    M = ax + gy.abs()

    def m(dy, dx):
        return _taps(M, dy, dx, False)

    t22 = ax * 13573
    t67 = t22 + (ax << 16)
    horiz = (M > m(0, -1)) & (M >= m(0, 1))
    vert = (M > m(-1, 0)) & (M >= m(1, 0))
    neg = (gx ^ gy) < 0  # s = -1
    diag = torch.where(neg,
                       (M > m(-1, 1)) & (M > m(1, -1)),
                       (M > m(-1, -1)) & (M > m(1, 1)))
    keep = torch.where(ay < t22, horiz, torch.where(ay > t67, vert, diag))
    thr = thr.to(device=M.device, dtype=torch.int32)
    cand = keep & (M > thr[:, 0].view(-1, 1, 1))
    E = keep & (M > thr[:, 1].view(-1, 1, 1))
    for _ in range(reach):
        grown = cand & (F.max_pool2d(E.to(torch.float32), 3, 1, 1) > 0)
        if torch.equal(grown, E):  # a fixed point: later passes change nothing
            break
        E = grown
    return E


def canny_hint(frames_u8: torch.Tensor, thr, reach: int = 16,
               dtype: torch.dtype = torch.float16,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """Edge hint for an edge ControlNet: (B,H,W,3) u8 RGB -> (B,H,W,3) of
    `dtype` (float16 or float32), the three channels equal, 1.0 on an edge
    and 0.0 elsewhere. The operator is defined in the comment above; any
    H, W >= 1.

    thr: (B,2) int32 tensor of (low, high) per row on the frames' device, or
    a pair of ints (validated, then broadcast into such a tensor). The
    kernel reads the tensor from memory, so a captured graph follows
    in-place writes to it. reach: 0..32 hysteresis steps, a launch constant.

    GPU: ONE launch of canny_hint (ops/csrc/canny.hip) on the current
    stream; the only allocation is `out` when it is not given, no sync.
    CPU tensors and AIRTC_FORCE_EAGER=1 take canny_hint_reference."""
    if frames_u8.dtype != torch.uint8:
        raise TypeError("canny_hint takes uint8 frames")
    if frames_u8.dim() != 4 or frames_u8.shape[-1] != 3 or frames_u8.numel() == 0:
        raise ValueError(
            f"canny_hint needs frames (B,H,W,3), got {tuple(frames_u8.shape)}")
    if dtype not in (torch.float16, torch.float32):
        raise TypeError(f"canny_hint writes float16 or float32, got {dtype}")
    if isinstance(reach, bool) or not isinstance(reach, int) \
            or not 0 <= reach <= CANNY_MAX_REACH:
        raise ValueError(
            f"reach must be an int in [0, {CANNY_MAX_REACH}], got {reach!r}")
    B = frames_u8.shape[0]
    if not isinstance(thr, torch.Tensor):
        if len(thr) != 2:
            raise ValueError("thr must be a (low, high) pair or a (B,2) tensor")
        lo, hi = check_canny_thresholds(*thr)
        thr = torch.tensor([[lo, hi]] * B, dtype=torch.int32,
                           device=frames_u8.device)
    if thr.dtype != torch.int32 or tuple(thr.shape) != (B, 2) \
            or thr.device != frames_u8.device:
        raise ValueError(
            f"thr must be a ({B}, 2) int32 tensor on {frames_u8.device}, got "
            f"{thr.dtype} {tuple(thr.shape)} on {thr.device}")
    if out is not None and (
            out.dtype != dtype or out.shape != frames_u8.shape
            or out.device != frames_u8.device or not out.is_contiguous()):
        raise ValueError(
            f"out must be a contiguous {dtype} {tuple(frames_u8.shape)} tensor "
            f"on {frames_u8.device}")
    if _use_hip(frames_u8, None):
        if out is None:
            out = torch.empty(frames_u8.shape, dtype=dtype, device=frames_u8.device)
        return _require_ext().canny_hint(
            frames_u8.contiguous(), thr.contiguous(), reach, out)
    E = canny_hint_reference(frames_u8, thr, reach)
    res = E.unsqueeze(-1).expand(-1, -1, -1, 3).to(dtype)
    if out is not None:
        out.copy_(res)
        return out
    return res.contiguous()


# ---------------------------------------------------------------------------
# YUV 4:2:0 frames (ops/csrc/color.hip)
# ---------------------------------------------------------------------------
# The frame format, stated once for the whole package:
#
# An I420 frame is a 2-D contiguous uint8 tensor of shape (3*H/2, W), H and W
# even: the first H*W bytes are the Y plane, the next (H/2)*(W/2) bytes Cb,
# the last (H/2)*(W/2) bytes Cr. All three planes are tight; the chroma
# planes are flat bytes inside the (H/2, W) tail (H need not be a multiple of
# 4). A batch is (B, 3*H/2, W). The dimensionality tells the formats apart:
# (H, W, 3) / (B, H, W, 3) is packed RGB, (3H/2, W) / (B, 3H/2, W) is I420
# (W is even, so a trailing dimension of 3 is always RGB).
#
# The arithmetic is the software codec's (ops/csrc/h264sw.cpp), BT.601
# limited range in integers, so every conversion below is bit-exact between
# the HIP kernels, the torch reference and the codec:
#   Y  = clip8(((66R + 129G + 25B + 128) >> 8) + 16)             per pixel
#   R' = (a+b+c+d+2) >> 2 per channel over each 2x2 block, then
#   Cb = clip8(((-38R' - 74G' + 112B' + 128) >> 8) + 128)
#   Cr = clip8(((112R' - 94G' - 18B' + 128) >> 8) + 128)
# and back, chroma nearest-replicated (Cb[y/2][x/2]), C=Y-16, D=Cb-128,
# E=Cr-128:
#   R = clip8((298C + 409E + 128) >> 8)
#   G = clip8((298C - 100D - 208E + 128) >> 8)
#   B = clip8((298C + 516D + 128) >> 8)
# (>> is an arithmetic shift: floor division by 256).

def is_i420(t: torch.Tensor) -> bool:
    """True when `t` has the shape and dtype of an I420 frame or batch."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        return False
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[-1] == 3):
        return False
    rows, w = int(t.shape[-2]), int(t.shape[-1])
    return rows >= 3 and rows % 3 == 0 and w >= 2 and w % 2 == 0


def i420_size(t: torch.Tensor) -> tuple:
    """(H, W) of the picture an I420 frame or batch holds."""
    _check_i420(t)
    return int(t.shape[-2]) // 3 * 2, int(t.shape[-1])


def _check_i420(t: torch.Tensor) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(
            f"I420 frames are uint8 tensors, got {getattr(t, 'dtype', type(t))}")
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[-1] == 3):
        raise ValueError(
            f"I420 frames are (3H/2, W) or (B, 3H/2, W), got {tuple(t.shape)}")
    if not is_i420(t):
        raise ValueError(
            f"I420 needs even H, W >= 2 in (3H/2, W), got {tuple(t.shape)}")


def _check_rgb_for_i420(x: torch.Tensor, dtype: torch.dtype | None) -> None:
    if dtype is not None and x.dtype != dtype:
        raise ValueError(f"expected {dtype}, got {x.dtype}")
    if dtype is None and not x.dtype.is_floating_point:
        raise ValueError(f"expected a floating-point image, got {x.dtype}")
    if x.dim() not in (3, 4) or x.shape[-1] != 3:
        raise ValueError(
            f"expected (H,W,3) or (B,H,W,3), got {tuple(x.shape)}")
    h, w = int(x.shape[-3]), int(x.shape[-2])
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f"I420 needs even H, W >= 2, got {h}x{w}")


def _clip8(v: torch.Tensor) -> torch.Tensor:
    return v.clamp(0, 255).to(torch.uint8)


def _rgb_u8_to_i420_ref(x: torch.Tensor) -> torch.Tensor:
    """(B,H,W,3) u8 -> (B,3H/2,W) u8 with the integer formulas above."""
    b, h, w, _ = x.shape
    p = x.to(torch.int32)
    r, g, bl = p[..., 0], p[..., 1], p[..., 2]
    y = _clip8(torch.bitwise_right_shift(66 * r + 129 * g + 25 * bl + 128, 8) + 16)
    q = p.reshape(b, h // 2, 2, w // 2, 2, 3).sum(dim=(2, 4))
    q = torch.bitwise_right_shift(q + 2, 2)
    r, g, bl = q[..., 0], q[..., 1], q[..., 2]
    cb = _clip8(torch.bitwise_right_shift(-38 * r - 74 * g + 112 * bl + 128, 8) + 128)
    cr = _clip8(torch.bitwise_right_shift(112 * r - 94 * g - 18 * bl + 128, 8) + 128)
    out = torch.cat([y.reshape(b, -1), cb.reshape(b, -1), cr.reshape(b, -1)], dim=1)
    return out.reshape(b, h // 2 * 3, w).contiguous()


def _i420_to_rgb_u8_ref(x: torch.Tensor) -> torch.Tensor:
    """(B,3H/2,W) u8 -> (B,H,W,3) u8 with the integer formulas above."""
    b, rows, w = x.shape
    h = rows // 3 * 2
    flat = x.reshape(b, -1).to(torch.int32)
    n, nc = h * w, (h // 2) * (w // 2)
    c = flat[:, :n].reshape(b, h, w) - 16

    def up(plane):
        plane = plane.reshape(b, h // 2, w // 2) - 128
        return plane.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)

    d, e = up(flat[:, n:n + nc]), up(flat[:, n + nc:])
    sh = torch.bitwise_right_shift
    r = _clip8(sh(298 * c + 409 * e + 128, 8))
    g = _clip8(sh(298 * c - 100 * d - 208 * e + 128, 8))
    bl = _clip8(sh(298 * c + 516 * d + 128, 8))
    return torch.stack([r, g, bl], dim=-1).contiguous()


def _batched(x: torch.Tensor, dims: int):
    """(x with a leading batch dim, whether one was added)."""
    return (x.unsqueeze(0), True) if x.dim() == dims else (x, False)


def _finish(res: torch.Tensor, out, squeeze: bool) -> torch.Tensor:
    if out is not None:
        return out
    return res[0] if squeeze else res


def _check_out(out, like: torch.Tensor, shape) -> None:
    if out is None:
        return
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) \
            or out.device != like.device or not out.is_contiguous():
        raise ValueError(
            f"out must be a contiguous uint8 {tuple(shape)} tensor on "
            f"{like.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")


def rgb_u8_to_i420(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """u8 RGB (H,W,3) / (B,H,W,3) -> I420 (3H/2,W) / (B,3H/2,W).

    GPU: one launch of the colour kernel on the current stream
    (non-contiguous input is made contiguous first). CPU tensors and
    AIRTC_FORCE_EAGER=1 take the torch integer reference. `out`, when given,
    is written in place (contiguous u8 of the result shape)."""
    _check_rgb_for_i420(x, torch.uint8)
    xb, squeeze = _batched(x, 3)
    b, h, w, _ = xb.shape
    ob = None if out is None else (out.unsqueeze(0) if squeeze else out)
    _check_out(ob, x, (b, h // 2 * 3, w))
    if _use_hip(x, None):
        res = _require_ext().rgb_u8_to_i420(xb.contiguous(), ob)
    else:
        res = _rgb_u8_to_i420_ref(xb)
        if ob is not None:
            ob.copy_(res)
    return _finish(res, out, squeeze)


def postprocess_to_i420(img: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Image (H,W,3) / (B,H,W,3) in [-1,1] -> I420, bit for bit
    rgb_u8_to_i420(postprocess_to_u8(img)).

    GPU f16: ONE kernel (postprocess_to_u8's rounding fused with the colour
    conversion, so the engine's decode graph gains no launch). Everything
    else (CPU, f32, AIRTC_FORCE_EAGER=1) composes the two references."""
    _check_rgb_for_i420(img, None)
    xb, squeeze = _batched(img, 3)
    b, h, w, _ = xb.shape
    ob = None if out is None else (out.unsqueeze(0) if squeeze else out)
    _check_out(ob, img, (b, h // 2 * 3, w))
    if _use_hip(img):
        res = _require_ext().postprocess_i420(xb.contiguous(), ob)
    else:
        u8 = (xb.float() + 1.0) * 127.5
        res = _rgb_u8_to_i420_ref(u8.round().clamp(0, 255).to(torch.uint8))
        if ob is not None:
            ob.copy_(res)
    return _finish(res, out, squeeze)


def unfit_geometry(Hs: int, Ws: int, H: int, W: int, mode: str = "cover",
                   even: bool = False, max_side: int = 0):
    """Inverse of fit_geometry: how a (H, W) engine frame goes back to a
    session that published (Hs, Ws).

    Returns ((ry, rx, rh, rw), (Ht, Wt)): the window of the engine frame to
    read and the size of the frame to hand back.
      stretch — whole frame, back to (Hs, Ws)
      contain — the ingest's destination window (the bars are cut away),
                back to (Hs, Ws)
      cover   — whole frame, back to the source window the ingest used
                (ch, cw); the cropped edges are not invented
    Then, in this order: max_side > 0 scales both sides so that the longer
    one is exactly max_side (only ever down), and `even` floors both sides
    to even, at least 2 (I420)."""
    (_, _, ch, cw), (oy, ox, oh, ow) = fit_geometry(Hs, Ws, H, W, mode)
    if max_side < 0:
        raise ValueError(f"max_side must be >= 0, got {max_side}")
    if mode == "contain":
        window, (Ht, Wt) = (oy, ox, oh, ow), (Hs, Ws)
    elif mode == "cover":
        window, (Ht, Wt) = (0, 0, H, W), (ch, cw)
    else:
        window, (Ht, Wt) = (0, 0, H, W), (Hs, Ws)
    longer = max(Ht, Wt)
    if max_side > 0 and longer > max_side:
        Ht, Wt = _round_div(Ht, max_side, longer), _round_div(Wt, max_side, longer)
    if even:
        Ht, Wt = max(2, Ht - Ht % 2), max(2, Wt - Wt % 2)
    return window, (Ht, Wt)


def unfit_frame_u8(img: torch.Tensor, window, size, fmt: str = "rgb",
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """Resize a window of one engine frame to a session's own size.

    img: (H, W, 3) u8 contiguous; window = (ry, rx, rh, rw) inside it;
    size = (Ht, Wt). fmt="rgb" returns (Ht, Wt, 3) u8, fmt="i420" returns
    the (3*Ht/2, Wt) I420 frame (Ht, Wt even) that is, bit for bit,
    rgb_u8_to_i420 of the RGB result. The filter is fit_frame_u8's:
    separable antialiased triangle, f32 accumulation, round-half-even,
    clamp, taps clamped to the window; an equal-size window is an exact
    copy. `out`, when given, is written in place.

    GPU: ONE launch on the current stream either way: fit_resize_u8 for RGB,
    fit_resize_u8_i420 (the same resize with the colour conversion done on
    the tile before it leaves the workgroup) for I420. CPU tensors and
    AIRTC_FORCE_EAGER=1 take the torch reference."""
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8:
        raise TypeError("unfit_frame_u8 takes a uint8 tensor")
    if img.dim() != 3 or img.shape[-1] != 3:
        raise ValueError(f"unfit_frame_u8 needs img (H,W,3), got {tuple(img.shape)}")
    if fmt not in ("rgb", "i420"):
        raise ValueError(f"fmt must be 'rgb' or 'i420', got {fmt!r}")
    H, W = int(img.shape[0]), int(img.shape[1])
    ry, rx, rh, rw = (int(v) for v in window)
    Ht, Wt = (int(v) for v in size)
    if min(rh, rw) < 1 or min(ry, rx) < 0 or ry + rh > H or rx + rw > W:
        raise ValueError(f"window {(ry, rx, rh, rw)} is not inside {(H, W)}")
    if min(Ht, Wt) < 1:
        raise ValueError(f"empty target size {(Ht, Wt)}")
    if fmt == "i420" and (Ht < 2 or Wt < 2 or Ht % 2 or Wt % 2):
        raise ValueError(f"I420 needs even H, W >= 2, got {Ht}x{Wt}")
    shape = (Ht, Wt, 3) if fmt == "rgb" else (Ht // 2 * 3, Wt)
    _check_out(out, img, shape)
    if _use_hip(img, None):
        if not img.is_contiguous():
            raise ValueError("img must be contiguous")
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=img.device)
        if fmt == "rgb":
            _require_ext().fit_resize_u8(img, out.unsqueeze(0), 0, ry, rx, rh,
                                         rw, 0, 0, Ht, Wt)
        else:
            _require_ext().fit_resize_u8_i420(img, out, ry, rx, rh, rw)
        return out
    win = _resize_u8_ref(img[ry:ry + rh, rx:rx + rw], Ht, Wt)
    # contiguous, and never a view of img
    res = win.clone(memory_format=torch.contiguous_format)
    if fmt == "i420":
        res = _rgb_u8_to_i420_ref(res.unsqueeze(0))[0]
    if out is None:
        return res
    out.copy_(res)
    return out


def i420_to_rgb_u8(x: torch.Tensor, H: int | None = None,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """I420 (3H/2,W) / (B,3H/2,W) -> u8 RGB (H,W,3) / (B,H,W,3).

    H is implied by the shape; pass it to have it checked. Dispatch and
    `out` as in rgb_u8_to_i420."""
    _check_i420(x)
    h, w = i420_size(x)
    if H is not None and H != h:
        raise ValueError(f"H={H} does not match the frame's {h} rows")
    xb, squeeze = _batched(x, 2)
    ob = None if out is None else (out.unsqueeze(0) if squeeze else out)
    _check_out(ob, x, (xb.shape[0], h, w, 3))
    if _use_hip(x, None):
        res = _require_ext().i420_to_rgb_u8(xb.contiguous(), ob)
    else:
        res = _i420_to_rgb_u8_ref(xb)
        if ob is not None:
            ob.copy_(res)
    return _finish(res, out, squeeze)


# ---------------------------------------------------------------------------
# CLIP safety checker (ops/csrc/safety.hip; models/safety_clip.py)
# ---------------------------------------------------------------------------
# The preprocessing, stated once. It is what CLIPImageProcessor does to the
# u8 frame the viewer would get, and the torch forms below are its
# definition (the HIP kernel computes the same thing in one launch):
#   1. every input pixel goes to the u8 level postprocess_to_u8 writes:
#      clamp(round_half_even((x + 1) * 127.5), 0, 255), in f32
#   2. resize so that the shorter side is `size`, the longer one
#      int(size * long / short): separable (horizontal, then vertical)
#      antialiased bicubic, Keys a = -0.5. Per axis scale = n_in / n_out,
#      fs = max(scale, 1), centre c = (o + 0.5) * scale, taps
#      [max(int(c - 2 fs + 0.5), 0), min(int(c + 2 fs + 0.5), n_in)), weight
#      k((j - c + 0.5) / fs) normalised to sum 1: the filter of PIL BICUBIC
#      and of F.interpolate(mode="bicubic", antialias=True,
#      align_corners=False). Nothing is rounded between the two passes (PIL
#      rounds to 8 bits there, so it differs by a few levels)
#   3. round half even, clamp to [0, 255]
#   4. centre crop size x size: top = (nh - size) // 2, left likewise
#   5. (v / 255 - mean_c) / std_c, evaluated in f64 per level and channel
#      and rounded once to f16 (a 3 x 256 table)
# and the result is laid out as the patch-embedding GEMM's A operand:
# (B, (size/patch)^2, 3 * patch^2), elements in (c, py, px) order.

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_geometry(H: int, W: int, size: int) -> tuple:
    """(nh, nw, top, left): the resized extent and the crop window in it."""
    short, long_ = (W, H) if W <= H else (H, W)
    new_long = int(size * long_ / short)
    nh, nw = (new_long, size) if W <= H else (size, new_long)
    return nh, nw, (nh - size) // 2, (nw - size) // 2


def _keys_cubic(x: torch.Tensor) -> torch.Tensor:
    x = x.abs()
    near = (1.5 * x - 2.5) * x * x + 1.0
    far = ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0
    return torch.where(x < 1.0, near, torch.where(x < 2.0, far, torch.zeros_like(x)))


def _aa_cubic_weights(n_in: int, n_out: int, first: int, count: int) -> torch.Tensor:
    """(count, n_in) f64: row i holds the normalised taps of output pixel
    first + i of an n_in -> n_out antialiased bicubic resize."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    c = (torch.arange(first, first + count, dtype=torch.float64) + 0.5) * scale
    start = (c - 2.0 * fs + 0.5).trunc().clamp_min(0)
    end = (c + 2.0 * fs + 0.5).trunc().clamp_max(n_in)
    j = torch.arange(n_in, dtype=torch.float64)
    w = _keys_cubic((j[None] - c[:, None] + 0.5) / fs)
    w = w * ((j[None] >= start[:, None]) & (j[None] < end[:, None]))
    return w / w.sum(dim=1, keepdim=True)


def clip_resize_reference(img: torch.Tensor, size: int = 224,
                          dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Steps 1, 2 and 4 above in `dtype` arithmetic: (B,H,W,3) in [-1,1] ->
    (B,size,size,3) levels BEFORE the rounding of step 3 (float64 is what
    the GPU tests hold the kernel against)."""
    _, H, W, _ = img.shape
    nh, nw, top, left = clip_geometry(H, W, size)
    u8 = ((img.float() + 1.0) * 127.5).round().clamp(0, 255)
    wx = _aa_cubic_weights(W, nw, left, size).to(device=img.device, dtype=dtype)
    wy = _aa_cubic_weights(H, nh, top, size).to(device=img.device, dtype=dtype)
    t = torch.einsum("ow,bhwc->bhoc", wx, u8.to(dtype))
    return torch.einsum("ph,bhoc->bpoc", wy, t)


_CLIP_LUT: dict = {}


def clip_lut(device) -> torch.Tensor:
    """(3, 256) f16: step 5 for every channel and level, cached per device."""
    device = torch.device(device)
    lut = _CLIP_LUT.get(device)
    if lut is None:
        v = torch.arange(256, dtype=torch.float64)[None] / 255.0
        mean = torch.tensor(CLIP_MEAN, dtype=torch.float64)[:, None]
        std = torch.tensor(CLIP_STD, dtype=torch.float64)[:, None]
        lut = ((v - mean) / std).to(torch.float16).contiguous().to(device)
        _CLIP_LUT[device] = lut
    return lut


def clip_levels_to_patches(levels: torch.Tensor, patch: int) -> torch.Tensor:
    """(B,size,size,3) integer levels -> (B, (size/patch)^2, 3*patch^2) f16."""
    B, size = levels.shape[0], levels.shape[1]
    g = size // patch
    lut = clip_lut(levels.device)
    vals = lut[torch.arange(3, device=levels.device), levels.long()]
    vals = vals.reshape(B, g, patch, g, patch, 3).permute(0, 1, 3, 5, 2, 4)
    return vals.reshape(B, g * g, 3 * patch * patch).contiguous()


def clip_patches(img: torch.Tensor, size: int = 224, patch: int = 14,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """Decoder image (B,H,W,3) f16/f32 in [-1,1] -> the CLIP tower's patch
    rows (B, (size/patch)^2, 3*patch^2) f16, by the preprocessing defined
    above. Any H, W >= 8; size a multiple of patch.

    GPU f16: ONE launch of clip_patches (ops/csrc/safety.hip) on the current
    stream; the only allocation is `out` when it is not given. Everything
    else (CPU, f32, AIRTC_FORCE_EAGER=1) takes the torch form."""
    if img.dim() != 4 or img.shape[-1] != 3 or not img.dtype.is_floating_point:
        raise ValueError(
            f"clip_patches needs a float image (B,H,W,3), got {img.dtype} "
            f"{tuple(img.shape)}")
    B, H, W, _ = img.shape
    if B < 1 or H < 8 or W < 8:
        raise ValueError(f"clip_patches needs B >= 1 and H, W >= 8, got {tuple(img.shape)}")
    if patch < 1 or size < patch or size % patch:
        raise ValueError(f"size must be a multiple of patch, got {size} and {patch}")
    g = size // patch
    shape = (B, g * g, 3 * patch * patch)
    if out is not None and (
            out.dtype != torch.float16 or tuple(out.shape) != shape
            or out.device != img.device or not out.is_contiguous()):
        raise ValueError(
            f"out must be a contiguous float16 {shape} tensor on {img.device}")
    if _use_hip(img):
        if out is None:
            out = torch.empty(shape, dtype=torch.float16, device=img.device)
        nh, nw, top, left = clip_geometry(H, W, size)
        return _require_ext().clip_patches(
            img.contiguous(), clip_lut(img.device), size, patch, nh, nw, top,
            left, out)
    levels = clip_resize_reference(img, size).round().clamp(0, 255)
    res = clip_levels_to_patches(levels, patch)
    if out is not None:
        out.copy_(res)
        return out
    return res


def quick_gelu(x: torch.Tensor) -> torch.Tensor:
    """x * sigmoid(1.702 x), CLIP's activation. GPU f16: vec8 kernel, f32
    math; shapes the vector path cannot read take the torch form."""
    if _use_hip(x) and x.numel() % 8 == 0:
        return _require_ext().quick_gelu(x.contiguous())
    xf = x.float()
    return (xf * torch.sigmoid(1.702 * xf)).to(x.dtype)


# The decision law of the reference StableDiffusionSafetyChecker, in order
# (cos against unit-norm rows; adj is its `adjustment`, positive = stricter):
#   special_j = cos_j - special_w_j + adj
#   care      = 0.01 if any(special_j > 0) else 0
#   concept_i = cos_i - concept_w_i + adj + care
#   flagged   = any(concept_i > 0)

def _unit_rows(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    t = t.detach().to(dtype)
    return (t / t.norm(dim=-1, keepdim=True)).contiguous()


def safety_head_reference(cls, ln_g, ln_b, proj_w, concept, concept_w,
                          special, special_w, adjust, eps: float = 1e-5,
                          dtype: torch.dtype = torch.float32):
    """LayerNorm -> projection -> cosines -> the law above, in `dtype`
    arithmetic. Returns (flags int32 (B,), scores `dtype` (B, ns + nc),
    special first)."""
    y = F.layer_norm(cls.to(dtype), (cls.shape[-1],), ln_g.to(dtype),
                     ln_b.to(dtype), eps)
    e = y @ proj_w.to(dtype).t()
    e = e / e.norm(dim=-1, keepdim=True)
    adj = adjust.to(dtype)[:, None]
    sp = e @ _unit_rows(special, dtype).t() - special_w.to(dtype)[None] + adj
    care = (sp > 0).any(dim=1, keepdim=True).to(dtype) * 0.01
    co = e @ _unit_rows(concept, dtype).t() - concept_w.to(dtype)[None] + adj + care
    flags = (co > 0).any(dim=1).to(torch.int32)
    return flags, torch.cat([sp, co], dim=1)


def safety_head(cls: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor,
                proj_w: torch.Tensor, concept: torch.Tensor,
                concept_w: torch.Tensor, special: torch.Tensor,
                special_w: torch.Tensor, adjust: torch.Tensor,
                counters: torch.Tensor, eps: float = 1e-5):
    """Everything after the tower, per frame: cls (B, hidden) class tokens
    -> (flags int32 (B,), scores f32 (B, n_special + n_concept)) by
    safety_head_reference, and counters[b] += flags[b] in place. adjust is
    (B,) f32 and counters (B,) int32, both read on the device: a captured
    graph follows in-place writes to them.

    GPU f16: ONE launch, one workgroup per frame (ops/csrc/safety.hip); f16
    cls and proj_w, f32 accumulation, nothing rounded to f16 on the way. The
    embedding tables are normalised once and cached on their tensors
    (weight_cache). Needs hidden % 8 == 0."""
    if adjust.dtype != torch.float32 or counters.dtype != torch.int32:
        raise TypeError("safety_head: adjust must be float32 and counters int32")
    if _use_hip(cls):
        ext = _require_ext()
        unit = lambda t: weight_cache(  # noqa: E731
            t, "_airtc_unit32", lambda: _unit_rows(t, torch.float32))
        flags, scores = ext.safety_head(
            cls, _f32(ln_g, "_airtc_g32"), _f32(ln_b, "_airtc_b32"), proj_w,
            unit(concept), _f32(concept_w, "_airtc_w32"), unit(special),
            _f32(special_w, "_airtc_w32"), adjust, counters, eps)
        return flags, scores
    flags, scores = safety_head_reference(
        cls, ln_g, ln_b, proj_w, concept, concept_w, special, special_w,
        adjust, eps)
    counters += flags
    return flags, scores.float()


def blank_flagged_(img: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """In place: frames b of img (B, ...) with flags[b] != 0 become -1
    (black) everywhere; the others are not written. No host sync."""
    if flags.dtype != torch.int32 or flags.numel() != img.shape[0]:
        raise ValueError("flags must be int32, one per frame")
    if _use_hip(img):
        if not img.is_contiguous():
            raise ValueError("img must be contiguous (it is written in place)")
        return _require_ext().blank_flagged_(img, flags)
    return img.masked_fill_(
        (flags != 0).view(-1, *([1] * (img.dim() - 1))), -1.0)


def lora_delta_(y: torch.Tensor, x: torch.Tensor, A: torch.Tensor,
                B: torch.Tensor, row_adapter: torch.Tensor,
                row_scale: torch.Tensor, col_offset: int = 0) -> torch.Tensor:
    """In place: y[b, :, col_offset : col_offset+N] += row_scale[b] *
    (x[b] @ A[a].T) @ B[a].T with a = row_adapter[b]; rows with a < 0 or
    a >= n and every other column of y are not written. x (Bt, L, K), y (Bt, L, Ny),
    A (n, R, K) "down", B (n, N, R) "up" (alpha/rank folded in), row_adapter
    (Bt,) int32, row_scale (Bt,) f32. Adapter and scale are read on the
    device: no host sync, and a captured graph follows later table writes.

    The torch form below defines the op: the intermediate is rounded to x's
    dtype, the scale multiplies the f32 second product, and the sum with y
    is rounded once. The HIP kernel (f16) refuses K % 32, N % 16,
    col_offset % 16, Ny % 4 != 0 and R outside {16, 32, 64}."""
    if x.dim() != 3 or y.dim() != 3 or A.dim() != 3 or B.dim() != 3:
        raise ValueError("lora_delta_: x (Bt, L, K), y (Bt, L, Ny), "
                         "A (n, R, K), B (n, N, R)")
    Bt, L, K = x.shape
    n, R, N = A.shape[0], A.shape[1], B.shape[1]
    if (y.shape[:2] != x.shape[:2] or A.shape[2] != K
            or B.shape[0] != n or B.shape[2] != R):
        raise ValueError(
            f"lora_delta_: shapes disagree: x {tuple(x.shape)}, y "
            f"{tuple(y.shape)}, A {tuple(A.shape)}, B {tuple(B.shape)}")
    if col_offset < 0 or col_offset + N > y.shape[2]:
        raise ValueError(
            f"lora_delta_: columns [{col_offset}, {col_offset + N}) do not "
            f"fit y's {y.shape[2]}")
    if (row_adapter.dtype != torch.int32 or row_adapter.shape != (Bt,)
            or row_scale.dtype != torch.float32 or row_scale.shape != (Bt,)):
        raise ValueError("lora_delta_: row_adapter (Bt,) int32 and "
                         "row_scale (Bt,) float32")
    if _use_hip(x):
        return _require_ext().lora_delta_(y, x, A, B, row_adapter, row_scale,
                                          int(col_offset))
    # an index past the bank is a row without an adapter, as in the kernel
    on = (row_adapter >= 0) & (row_adapter < n)
    idx = row_adapter.clamp(0, n - 1).long()
    t = torch.bmm(x, A[idx].transpose(1, 2))  # rounded to x's dtype
    d = torch.bmm(t.float(), B[idx].float().transpose(1, 2))
    ys = y[:, :, col_offset:col_offset + N]
    new = (ys.float() + row_scale.view(-1, 1, 1) * d).to(y.dtype)
    ys.copy_(torch.where(on.view(-1, 1, 1), new, ys))
    return y
