"""CPU checks of the streaming route choice of pfmi.api (_use_stream): which device-optimised runs take the streaming pipeline
(pfmi_stream_enqueue) -- built-in targets and device closures with a gradient, history_length <= 16, unless PFMI_NO_STREAM=1."""
import pytest


class _Dev:
    kind = 3

    def __init__(self, d, grad):
        self.d, self.has_device_gradient = d, grad


class _Builtin:
    def __init__(self, kind, d):
        self.kind, self.d = kind, d


class _Host:
    kind = 2
    d = 10


def test_gradient_closures_stream_like_builtin_targets(monkeypatch):
    from pfmi.api import _use_device_optimizer, _use_stream
    monkeypatch.delenv("PFMI_NO_STREAM", raising=False)
    t = _Dev(50_000, True)
    assert _use_stream(t, _use_device_optimizer(t, "auto", 6), 6)              # any d: the closure's round kernel walks memory
    assert _use_stream(_Dev(10, True), True, 16)
    assert not _use_stream(_Dev(10, True), True, 17)                          # the pipeline pads to 32 columns: J 17 .. 32 stay packed
    assert not _use_stream(_Dev(10, True), False, 6)                          # not optimised on the device: nothing to stream
    for kind in (0, 1):
        assert _use_stream(_Builtin(kind, 100), True, 16)
        assert not _use_stream(_Builtin(kind, 100), True, 17)


def test_no_gradient_and_host_closures_never_stream(monkeypatch):
    from pfmi.api import _use_stream
    monkeypatch.delenv("PFMI_NO_STREAM", raising=False)
    assert not _use_stream(_Dev(10, False), True, 6)
    assert not _use_stream(_Host(), True, 6)


@pytest.mark.parametrize("value,streams", [("1", False), ("0", True), ("", True)])
def test_no_stream_switch(monkeypatch, value, streams):
    from pfmi.api import _use_stream
    monkeypatch.setenv("PFMI_NO_STREAM", value)
    assert _use_stream(_Dev(10, True), True, 6) is streams
    assert _use_stream(_Builtin(0, 100), True, 6) is streams
