"""Host-side contract of the linear + residual epilogue path: one hipBLASLt
per process, and a dispatch that leaves the CPU and switched-off paths alone."""
import torch
import torch.nn.functional as F

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.ops import interface


def _inputs(dtype):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 16, generator=g).to(dtype)
    w = torch.randn(24, 16, generator=g).to(dtype)
    b = torch.randn(24, generator=g).to(dtype)
    r = torch.randn(2, 5, 24, generator=g).to(dtype)
    return x, w, b, r


def test_single_hipblaslt_in_process():
    """The extension links the hipBLASLt that torch loads: after importing
    both, the process maps exactly one libhipblaslt file."""
    ext = ops.hip_ext()
    assert ext is not None, "the HIP extension must be built"
    assert hasattr(ext, "linear_residual")
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libhipblaslt" in line}
    assert len(paths) == 1, paths


def test_cpu_path_untouched(monkeypatch):
    monkeypatch.delenv("AIRTC_LT_EPILOGUE", raising=False)
    for dtype in (torch.float32, torch.float16):
        x, w, b, r = _inputs(dtype)
        assert torch.equal(ops.linear(x, w, b, residual=r),
                           F.linear(x, w, b) + r)
        assert torch.equal(ops.linear(x, w, None, residual=r),
                           F.linear(x, w) + r)
        assert torch.equal(ops.linear(x, w, b), F.linear(x, w, b))


class _NoAttr:
    def __getattr__(self, name):
        raise AssertionError(f"extension attribute {name!r} was looked up")


def test_switch_off_never_touches_the_extension(monkeypatch):
    """AIRTC_LT_EPILOGUE=0: even tensors that would take the HIP path go to
    F.linear + add without a look at the extension."""
    monkeypatch.setenv("AIRTC_LT_EPILOGUE", "0")
    monkeypatch.delenv("AIRTC_FUSED_PROJ", raising=False)
    monkeypatch.setattr(interface, "hip_ext", lambda: _NoAttr())
    monkeypatch.setattr(interface, "_use_hip", lambda t: True)
    x, w, b, r = _inputs(torch.float16)
    assert torch.equal(ops.linear(x, w, b, residual=r), F.linear(x, w, b) + r)


def test_switch_on_looks_up_the_entry_point(monkeypatch):
    """The counterpart: with the switch at its default the same call does
    reach for the extension, so the test above checks the switch."""
    monkeypatch.delenv("AIRTC_LT_EPILOGUE", raising=False)
    monkeypatch.delenv("AIRTC_FUSED_PROJ", raising=False)
    seen = []

    class Ext:
        def linear_residual(self, x, w, b, r):
            seen.append(tuple(r.shape))
            return F.linear(x, w, b) + r

    monkeypatch.setattr(interface, "hip_ext", lambda: Ext())
    monkeypatch.setattr(interface, "_use_hip", lambda t: True)
    monkeypatch.setattr(interface, "_LT_SEEN", set())
    x, w, b, r = _inputs(torch.float16)
    ops.linear(x, w, b, residual=r)
    ops.linear(x, w, b, residual=r)
    assert seen == [(2, 5, 24)] * 2
