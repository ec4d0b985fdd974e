"""CPU checks of the device L-BFGS for user closures: the routing rules of pfmi.api._use_device_optimizer and the resource pin of the new
kernel (read from the gfx950 code objects of the library that was just built, as tests/test_kernel_resources.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))


class _Dev:
    kind = 3

    def __init__(self, d, grad):
        self.d, self.has_device_gradient = d, grad


class _Builtin:
    def __init__(self, kind, d):
        self.kind, self.d = kind, d


def test_routing_of_gradient_closure_targets():
    from pfmi.api import _use_device_optimizer
    for opt in ("auto", "device"):
        assert _use_device_optimizer(_Dev(50_000, True), opt, 6)          # any d
        assert _use_device_optimizer(_Dev(10, True), opt, 32)
    assert not _use_device_optimizer(_Dev(10, True), "auto", 33)
    with pytest.raises(ValueError):
        _use_device_optimizer(_Dev(10, True), "device", 33)
    assert not _use_device_optimizer(_Dev(10, True), "host", 6)
    # everything else routes as before
    assert not _use_device_optimizer(_Dev(10, False), "auto", 6)
    with pytest.raises(ValueError):
        _use_device_optimizer(_Dev(10, False), "device", 6)
    assert _use_device_optimizer(_Builtin(0, 100), "auto", 6)
    assert not _use_device_optimizer(_Builtin(0, 20_000), "auto", 6)
    assert not _use_device_optimizer(_Builtin(1, 100), "auto", 17)
    assert not _use_device_optimizer(_Builtin(2, 100), "auto", 6)


def test_torch_target_gradient_keyword():
    torch = pytest.importorskip("torch")
    import pfmi
    t0 = pfmi.TorchDeviceTarget(4, lambda X: -(X * X).sum(1))
    assert not t0.has_device_gradient and t0.gradient_pointer() is None
    t1 = pfmi.TorchDeviceTarget(4, lambda X: -(X * X).sum(1), grad="autograd")
    assert t1.has_device_gradient and t1.gradient_pointer()[0]
    with pytest.raises(ValueError):
        pfmi.TorchDeviceTarget(4, lambda X: X.sum(1), grad="finite-differences")
    del torch


def test_closure_lbfgs_kernel_has_no_scratch():
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    t = kr.kernel_resources()
    for prefix, vmax in (("pf_lbc_step_kernel(", 256), ("pf_lbc_init_kernel(", 64)):
        hits = [k for k in t if k.startswith(prefix)]
        assert len(hits) == 1, (prefix, hits)
        r = t[hits[0]]
        assert r["vgpr_count"] <= vmax, (hits[0], r)
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (hits[0], r)
