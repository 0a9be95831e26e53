"""Helpers of tests/test_gpu_streams.py: a context on a non-blocking side stream, ballast in front of a race, the serial reference.

A race between a library call and the work enqueued before it is made deterministic by putting BALLAST in front of that work: a spin
kernel of known length on the stream.  While the ballast runs, everything enqueued behind it on that stream has provably not happened
yet (`event.query()` of the event recorded behind the ballast is False), so a call that must wait for it, or must not, shows which it
did.  The reference of every test is `serial()`: the same call sequence in a context on the null stream with a device synchronise
after every call -- the configuration the rest of the suite pins to the oracle.
"""
import contextlib
import ctypes

import numpy as np

NOMINAL_MS = 100.0             # ballast in front of one group of calls
HIP_STREAM_NON_BLOCKING = 1    # hipStreamNonBlocking

_hip = None
_cycles_per_ms = None


def hip_runtime():
    """The HIP runtime this process has already mapped (torch's copy serves the library too), by its path in the process's map."""
    global _hip
    if _hip is None:
        import torch  # noqa: F401  (maps it)
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "libamdhip64 is not mapped into this process"
        _hip = ctypes.CDLL(path)
        _hip.hipStreamGetFlags.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
        _hip.hipStreamGetFlags.restype = ctypes.c_int
    return _hip


def side_stream():
    """A torch side stream, checked to be what the whole file rests on: a real stream (not the null stream) that is NON-BLOCKING, i.e.
    not ordered against the null stream the library's blocking copies and (formerly) fills run on."""
    import torch
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0, "torch.cuda.Stream() returned the null stream"
    flags = ctypes.c_uint(0xffffffff)
    rc = hip_runtime().hipStreamGetFlags(ctypes.c_void_p(s.cuda_stream), ctypes.byref(flags))
    assert rc == 0, "hipStreamGetFlags failed: %d" % rc
    assert flags.value & HIP_STREAM_NON_BLOCKING, "torch's side stream is a blocking stream (flags %#x): these tests would order nothing" % flags.value
    return s


def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond of the event clock, measured once per session (never against the code under test)."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch
        torch.cuda.synchronize()
        cycles, ms = 1000000, 0.0
        for _ in range(8):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 20.0:
                break
            cycles *= 4
        assert ms >= 20.0, "torch.cuda._sleep(%d) took %.3f ms: it does not spin on this device" % (cycles, ms)
        _cycles_per_ms = cycles / ms
        print("stream_ballast: %.0f _sleep cycles per ms (%d cycles took %.2f ms)" % (_cycles_per_ms, cycles, ms))
    return _cycles_per_ms


def ballast(stream, ms=NOMINAL_MS):
    """Enqueues a spin of `ms` milliseconds on `stream`; returns the event recorded behind it."""
    import torch
    n = int(ms * cycles_per_ms())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(n)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def bits(a):
    """An array as its 32-bit words: equality of these is bit-equality (NaN payloads and signed zeros included)."""
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 4:
        return a.view(np.uint32)
    return np.frombuffer(a.tobytes(), np.uint8)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def differing_pixels(a, b):
    """Fraction of the pixels of two (H, W, C) images of which any bit differs."""
    return float((bits(a) != bits(b)).any(axis=-1).mean())


class Synced:
    """A Renderer whose every call is followed by a device synchronise."""

    def __init__(self, r):
        self.__dict__["_r"] = r

    def __getattr__(self, name):
        v = getattr(self._r, name)
        if not callable(v):
            return v

        def call(*a, **kw):
            import torch
            out = v(*a, **kw)
            torch.cuda.synchronize()
            return out
        return call

    def __setattr__(self, name, value):
        setattr(self._r, name, value)


class Env:
    """What a flow (a function of one Env) is run in: `streams[k] is None` = the serial reference."""

    def __init__(self, streams, total_ms_limit=2000.0):
        self.streams = streams
        self.serial = streams[0] is None
        self.spent_ms = 0.0
        self.limit = total_ms_limit
        self.renderers = []

    def stream(self, k=0):
        import torch
        return torch.cuda.stream(self.streams[k]) if not self.serial else contextlib.nullcontext()

    def R(self, k=0):
        """A context on stream k (serial: on the null stream, synchronised after every call)."""
        import torch
        from gltf_renderer_amd.renderer import Renderer
        if self.serial:
            r = Synced(Renderer(0, stream=0))
            torch.cuda.synchronize()
        else:
            r = Renderer(0, stream=self.streams[k].cuda_stream)
        self.renderers.append(r)
        return r

    def ballast(self, ms=NOMINAL_MS, k=0, stream=None):
        """Ballast on stream k (or the stream given); None in the serial run."""
        if self.serial:
            return None
        self.spent_ms += ms
        assert self.spent_ms <= self.limit, "more than %.0f ms of ballast in one test" % self.limit
        return ballast(self.streams[k] if stream is None else stream, ms)

    def open(self, ev, what):
        """The premise: the ballast is still running, so nothing enqueued behind it has happened."""
        if ev is not None:
            assert not ev.query(), "premise failed: the ballast had run out before / when %s returned -- the race window is closed" % what

    def sync(self):
        import torch
        if self.serial:
            torch.cuda.synchronize()
        else:
            for s in self.streams:
                s.synchronize()

    def close(self):
        import torch
        torch.cuda.synchronize()
        for r in self.renderers:
            r.close()
        self.renderers = []


def serial(fn, *args):
    """The reference: fn's call sequence on the null stream with a synchronise after every call."""
    import torch
    torch.cuda.synchronize()
    env = Env([None])
    try:
        return fn(env, *args)
    finally:
        env.close()


def on_streams(fn, streams, *args):
    """fn's call sequence with its contexts on the given side streams; torch's own work (allocation fills, poison) goes on streams[0]."""
    import torch
    torch.cuda.synchronize()
    env = Env(list(streams))
    try:
        with torch.cuda.stream(streams[0]):
            return fn(env, *args)
    finally:
        env.close()
