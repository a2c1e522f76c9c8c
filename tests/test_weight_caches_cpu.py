"""ops.weight_cache / ops.drop_weight_caches on their own, and
refresh_weights on a CPU engine."""
import torch
from torch import nn

from ai_rtc_agent_amd import ops
from ai_rtc_agent_amd.engine import StreamDiffusionEngine


def registered_attrs(module):
    """(owner, name) of every registered cache attribute left in the tree."""
    left = []
    for m in module.modules():
        for owner in (m, *m.parameters(recurse=False)):
            left += [(owner, n) for n in ops.weight_cache_names()
                     if hasattr(owner, n)]
    return left


def test_registers_builds_once_and_drops():
    lin = nn.Linear(4, 4)
    calls = []

    def build():
        calls.append(1)
        return lin.weight.detach() * 2

    a = ops.weight_cache(lin.weight, "_airtc_test_double", build)
    b = ops.weight_cache(lin.weight, "_airtc_test_double", build)
    assert a is b and len(calls) == 1
    assert "_airtc_test_double" in ops.weight_cache_names()
    assert hasattr(lin.weight, "_airtc_test_double")
    # a module can own an entry as well as a parameter
    ops.weight_cache(lin, "_test_fused", lambda: lin.weight.detach().t())
    assert len(registered_attrs(lin)) == 2
    ops.drop_weight_caches(nn.Sequential(lin))
    assert registered_attrs(lin) == []
    c = ops.weight_cache(lin.weight, "_airtc_test_double", build)
    assert len(calls) == 2 and c is not a


def test_secondary_key():
    w = nn.Parameter(torch.ones(3))
    t1, t2 = torch.zeros(3), torch.zeros(3)  # equal values, two tensors
    n = []

    def build():
        n.append(1)
        return torch.full((3,), float(len(n)))

    # tensors key by identity
    a = ops.weight_cache(w, "_airtc_test_keyed", build, key=t1)
    assert ops.weight_cache(w, "_airtc_test_keyed", build, key=t1) is a
    b = ops.weight_cache(w, "_airtc_test_keyed", build, key=t2)
    assert b is not a and len(n) == 2
    # tuples elementwise, None included
    c = ops.weight_cache(w, "_airtc_test_keyed", build, key=(t1, None))
    assert ops.weight_cache(w, "_airtc_test_keyed", build, key=(t1, None)) is c
    assert ops.weight_cache(w, "_airtc_test_keyed", build, key=(t1, t2)) is not c
    # plain values by equality
    d = ops.weight_cache(w, "_airtc_test_keyed", build, key=0.5)
    assert ops.weight_cache(w, "_airtc_test_keyed", build, key=0.5) is d
    assert ops.weight_cache(w, "_airtc_test_keyed", build, key=0.25) is not d


def test_refresh_weights_leaves_no_registered_attribute(tiny_cfg):
    e = StreamDiffusionEngine(tiny_cfg)
    e.prepare()
    g = torch.Generator().manual_seed(0)
    e(torch.randint(0, 256, (64, 64, 3), generator=g, dtype=torch.uint8))
    modules = [m for m in (e.unet, e.vae, e.controlnet) if m is not None]
    # the attention modules cache their fused projections on the CPU too
    before = {(id(o), n): getattr(o, n)
              for m in modules for o, n in registered_attrs(m)}
    assert before
    e.refresh_weights()
    # no entry from before the refresh is left. The only names present are
    # the K|V projections that refresh_weights' own static-K/V pass has just
    # rebuilt from the new weights.
    for m in modules:
        for o, n in registered_attrs(m):
            assert n == "_wkv" and getattr(o, n) is not before[(id(o), n)]
