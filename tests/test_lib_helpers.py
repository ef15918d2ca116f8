"""The device-call helpers of expecto_amd/_lib.py, without a library or a device: ``_lib.load`` returns a stub."""
import numpy as np
import pytest

from expecto_amd import _lib


class StubLib:
    """Entry points that record their arguments and return ``status``."""

    def __init__(self, status=0, message="bad things"):
        self.status, self.message, self.calls = status, message, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.status
        return entry

    def expecto_last_error(self):
        return self.message.encode()


@pytest.fixture
def stub(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0xBEEF)
    return lib


def test_call_appends_one_stream_and_raises_the_library_message(stub):
    _lib.call("expecto_x", 1, None, 2.5)
    assert stub.calls == [("expecto_x", (1, None, 2.5, 0xBEEF))]
    stub.status = -3
    with pytest.raises(RuntimeError) as e:
        _lib.call("expecto_x", 7)
    assert str(e.value) == "expecto_x failed (status -3): bad things"
    with pytest.raises(RuntimeError) as e:
        _lib.call("expecto_x", 7, what="x")
    assert str(e.value) == "x failed (status -3): bad things"
    assert stub.calls[1:] == [("expecto_x", (7, 0xBEEF))] * 2


def test_host_call_appends_no_stream_and_raises_in_both_formats(stub):
    _lib.host_call("expecto_h", 1, 2)
    assert stub.calls == [("expecto_h", (1, 2))]
    stub.status = -1
    with pytest.raises(ValueError) as e:
        _lib.host_call("expecto_h", 1)
    assert str(e.value) == "expecto_h: bad things"
    with pytest.raises(ValueError) as e:
        _lib.host_call("expecto_h", 1, prefix=False)
    assert str(e.value) == "bad things"


def test_require_gpu_raises_the_sentence(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError) as e:
        _lib.require_gpu("x")
    assert str(e.value) == "expecto_amd.x needs a GPU (HIP); there is no CPU path"
    with pytest.raises(RuntimeError) as e:
        _lib.require_gpu("x", " to cluster")
    assert str(e.value) == "expecto_amd.x needs a GPU (HIP) to cluster; there is no CPU path"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert _lib.require_gpu("x") is torch


def test_device_of_keeps_a_given_device():
    import torch
    assert _lib.device_of("cuda:3") == torch.device("cuda", 3)
    assert _lib.device_of(torch.device("cuda", 1)) == torch.device("cuda", 1)


def test_upload_and_workspace_on_the_host():
    import torch
    a = np.arange(12, dtype=np.int32).reshape(3, 4)[:, ::2]           # not contiguous
    t = _lib.upload(a, "cpu")
    assert t.is_contiguous() and t.dtype == torch.int32 and np.array_equal(t.numpy(), a)
    for nbytes, numel in ((0, 0), (1, 1), (8, 1), (9, 2), (4096, 512)):
        ws = _lib.workspace(nbytes, "cpu")
        assert ws.dtype == torch.float64 and ws.numel() == numel


def test_event_timer_without_timings_constructs_no_event(monkeypatch):
    import torch

    def no_event(*a, **k):
        raise AssertionError("an event was constructed")
    monkeypatch.setattr(torch.cuda, "Event", no_event)
    timer = _lib.EventTimer(None)
    timer.mark()
    timer.mark(sync=True)
    timer.mark()
    timer.set("a_ms")
    timer.add("b_ms", 1)
    assert timer.events == [] and timer.timings is None


def test_event_timer_sets_and_accumulates_intervals(monkeypatch):
    import torch

    class FakeEvent:
        clock = 0.0

        def __init__(self, enable_timing=False):
            assert enable_timing
            self.at, self.synced = None, False

        def record(self):
            FakeEvent.clock += 1.5
            self.at = FakeEvent.clock

        def synchronize(self):
            self.synced = True

        def elapsed_time(self, other):
            return other.at - self.at
    monkeypatch.setattr(torch.cuda, "Event", FakeEvent)
    timings = {"sum_ms": 10.0}
    timer = _lib.EventTimer(timings)
    timer.mark()
    timer.mark()
    FakeEvent.clock += 2.0
    timer.mark(sync=True)
    assert [e.synced for e in timer.events] == [False, False, True]
    timer.set("first_ms")
    timer.set("second_ms", 1)
    timer.add("sum_ms", 1)
    timer.add("new_ms")
    assert timings == {"sum_ms": 13.5, "first_ms": 1.5, "second_ms": 3.5, "new_ms": 1.5}
