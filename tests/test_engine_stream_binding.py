"""CPU tier: the Engine binds a context slot to torch's current stream and launches in two separate library calls.  Torch's
current stream is thread-local and ctypes drops the GIL, so two threads on one Engine, each under its own stream, must not be
able to interleave one thread's bind with the other's launch: the kernel would run on the wrong stream, unordered with its
consumers and with the memory torch.empty handed out for the right one.

No GPU and no native library here: `Engine(lib=...)` gets a stub that records the stream last bound to the slot
(zc_ctx_set_stream_dev), yields for about a millisecond at the end of every bind to widen the window, and checks in every entry
point that the bound stream is the calling thread's.  Tensors, torch.empty and torch.cuda.current_stream are thread-local fakes."""
import threading
import time

import numpy as np
import pytest

from dusk_zerocaf_amd import engine as E

CALLS_PER_THREAD = 200
BIND_YIELD_S = 0.001


class FakeDevice:
    type, index = "cuda", 0


class FakeTensor:
    """What Engine reads of a contiguous torch CUDA tensor."""
    _next_ptr = [0x10000]

    def __init__(self, shape, dtype=None, itemsize=8):
        self.shape, self.dtype, self._itemsize, self.device = tuple(shape), dtype, itemsize, FakeDevice()
        self._ptr = FakeTensor._next_ptr[0]
        FakeTensor._next_ptr[0] += 0x1000

    def data_ptr(self): return self._ptr
    def is_contiguous(self): return True
    def element_size(self): return self._itemsize


class StubLib:
    """The ABI as Engine sees it.  Every zc_* entry point that is not a context call is a launch: it must find the slot bound to
    the stream of the thread that makes it (`current`: thread-local, set by the test)."""

    def __init__(self, current):
        self.current = current
        self.bound = None                 # what the slot's stream is: None = the context's own
        self.binds = 0
        self.launches = []                # (entry point, bound stream, the caller's stream)
        self.wrong = []                   # the launches that ran on another thread's stream

    def zc_ctx_create(self, devices, ndev, out): return 0
    def zc_ctx_destroy(self, ctx): return 0
    def zc_ctx_device_count(self, ctx): return 1
    def zc_ctx_device(self, ctx, slot): return 0
    def zc_ctx_synchronize(self, ctx): return 0
    def zc_last_error(self): return b""

    def zc_ctx_set_stream_dev(self, ctx, slot, stream, external):
        self.bound = stream.value if external else None
        self.binds += 1
        time.sleep(BIND_YIELD_S)          # the window between a bind and its launch, held open
        return 0

    def zc_ctx_set_stream(self, ctx, stream, external):
        return self.zc_ctx_set_stream_dev(ctx, 0, stream, external)

    def __getattr__(self, name):
        if not name.startswith("zc_"):
            raise AttributeError(name)

        def launch(ctx, *args):
            mine = getattr(self.current, "handle", None)
            self.launches.append((name, self.bound, mine))
            if mine is not None and self.bound != mine:
                self.wrong.append((name, "bound %#x" % (self.bound or 0), "caller %#x" % mine, threading.current_thread().name))
                raise AssertionError("%s launched on stream %#x, the calling thread's current stream is %#x" % (name, self.bound or 0, mine))
            return 0
        return launch


@pytest.fixture
def stubbed(monkeypatch):
    """(engine on the stub, the stub, thread-local holder of the calling thread's stream handle)"""
    import torch
    current = threading.local()

    class FakeStream:
        def __init__(self, handle): self.cuda_stream = handle

    monkeypatch.setattr(E, "_is_torch", lambda x: isinstance(x, FakeTensor))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: FakeStream(current.handle))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch, "empty", lambda shape, dtype=None, device=None: FakeTensor(shape, dtype, 1 if dtype == torch.uint8 else 8))
    stub = StubLib(current)
    eng = E.Engine(devices=[0], lib=stub)
    return eng, stub, current


def _mixed_calls(eng, i):
    """a one-output op, a two-output op and msm_partial, which binds through its output"""
    a, b = FakeTensor((64, 5)), FakeTensor((64, 5))
    if i % 3 == 0:
        out = eng.fe_mul(a, b)
        assert isinstance(out, FakeTensor) and out.shape == (64, 5)
    elif i % 3 == 1:
        out, ok = eng.fe_invert(a)
        assert out.shape == (64, 5) and ok.shape == (64,)
    else:
        out = eng.msm_partial(FakeTensor((64, 20)), b)
        assert out.shape == (1, 20)


def test_two_threads_with_their_own_streams_never_launch_on_each_others(stubbed):
    """Two threads, 200 calls each, each thread under its own current stream: every launch finds the slot bound to the stream
    of the thread that makes it.  (Without a lock over bind + allocate + launch the first calls already fail: thread B rebinds
    the slot while thread A sits between its bind and its launch.)"""
    eng, stub, current = stubbed
    errors = []
    start = threading.Barrier(2)

    def worker(handle):
        current.handle = handle
        start.wait()
        for i in range(CALLS_PER_THREAD):
            try:
                _mixed_calls(eng, i)
            except AssertionError as e:
                errors.append(str(e))

    threads = [threading.Thread(target=worker, args=(h,), name="stream-%#x" % h) for h in (0xA000, 0xB000)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    print("binds: %d, launches: %d, launches on another thread's stream: %d" % (stub.binds, len(stub.launches), len(stub.wrong)))
    assert len(stub.launches) == 2 * CALLS_PER_THREAD
    assert not stub.wrong, "%d of %d launches ran on the other thread's stream, the first: %s" % (len(stub.wrong), len(stub.launches), stub.wrong[0])
    assert not errors, errors[:3]
    assert {s for _, s, _ in stub.launches} == {0xA000, 0xB000}


def test_a_pinned_stream_is_never_rebound(stubbed):
    """After set_stream() nothing follows torch: calls on tensors from any thread's current stream leave the binding alone;
    use_own_stream() gives the following back."""
    eng, stub, current = stubbed
    eng.set_stream(0xC000)
    assert stub.bound == 0xC000 and stub.binds == 1
    current.handle = None                 # the launches are not checked against a thread's stream: the pin decides
    for i in range(6):
        _mixed_calls(eng, i)
    assert stub.binds == 1 and {s for _, s, _ in stub.launches} == {0xC000}
    eng.use_own_stream()
    assert stub.bound is None and stub.binds == 2
    current.handle = 0xD000
    _mixed_calls(eng, 0)
    assert stub.bound == 0xD000 and stub.binds == 3
    _mixed_calls(eng, 1)                  # the same stream again: no second bind
    assert stub.binds == 3


def test_host_array_calls_bind_nothing(stubbed):
    """numpy inputs are staged by the library on the context's stream: the Engine binds nothing for them."""
    eng, stub, current = stubbed
    current.handle = None
    a = np.zeros((4, 5), dtype=np.uint64)
    out = eng.fe_mul(a, a)
    inv, ok = eng.fe_invert(a)
    assert isinstance(out, np.ndarray) and out.shape == (4, 5) and ok.shape == (4,)
    assert stub.binds == 0 and [name for name, _, _ in stub.launches] == ["zc_fe_mul", "zc_fe_invert"]
