"""Holding a stream back, so that a test can see who waits for whom (tests/test_gpu_stream_order.py).

hold(stream, ms) queues a bounded spin (torch.cuda._sleep: one workgroup that reads the clock until `cycles` have passed) on `stream` and
returns an event recorded behind it. Work queued behind the hold cannot start for `ms` milliseconds, so whatever the host submits in that
time to ANOTHER stream runs first unless something orders it -- which is what the tests pin. Without a hold every piece of work of a small
scene is over long before the host submits the next one, and a missing wait shows nowhere.

The length of a hold is a condition of every case, not an assumption: Hold.must_be_pending() is called right after the last call a case
placed in the window and fails the case, saying so, when the hold had already ended by then.

Measured on an MI355X (HOLD_MS was chosen from these; Hold.must_be_pending prints each case's window, WINDOWS collects them):
    torch.cuda._sleep counts                            2.35 - 2.38 million cycles per millisecond (1 000 000 cycles took 0.42 ms)
    windows, hold() to the last racing call's return    0.16 - 1.31 ms over the 24 cases of tests/test_gpu_stream_order.py in three runs; the
                                                        longest: a held shade_rays, an instance upload, a frame in flight, a trace_rays
    HOLD_MS                                             100: 76 times the longest window; the spare costs a tenth of a second a case
A window is this short only when nothing in it allocates: a case runs every call of its window once, unheld, beforehand. (Left in the window, the
first frame in flight of a session returned only when the hold was over -- 98.8 to 99.2 ms -- and the cases said so.)

Two HIP streams may share a hardware queue (the runtime deals streams over GPU_MAX_HW_QUEUES queues), and then work on one is serialised
behind a hold on the other whether or not anything orders it, which would hide a missing wait. independent() is the control: it runs a
case's attempt on up to MAX_ATTEMPTS fresh side streams until the operation that must NOT be ordered behind the hold completed while the
hold was pending; if none does, the case fails as inconclusive. A case holds once per attempt: at most MAX_ATTEMPTS * HOLD_MS = 0.8 s.
"""
import functools
import time

import pytest

HOLD_MS = 100.0
MAX_ATTEMPTS = 8
CALIBRATION_CYCLES = 1_000_000
WINDOWS = []                    # (case, milliseconds from hold() to the last call in the window) of every must_be_pending() of this process


@functools.lru_cache(maxsize=None)
def cycles_per_ms():
    """what torch.cuda._sleep counts per millisecond: one short spin between two timing events, once per process"""
    import torch
    torch.cuda._sleep(1000)                                  # the kernel's first launch loads it
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    torch.cuda._sleep(CALIBRATION_CYCLES)
    end.record()
    end.synchronize()
    ms = start.elapsed_time(end)
    assert ms > 0.05, f"torch.cuda._sleep({CALIBRATION_CYCLES}) took {ms} ms: too short to calibrate a hold with"
    rate = CALIBRATION_CYCLES / ms
    print(f"stream_hold: torch.cuda._sleep counts {rate:.0f} cycles per ms ({CALIBRATION_CYCLES} cycles took {ms:.3f} ms)")
    return rate


def hold(stream, ms):
    """Queue a spin of `ms` milliseconds on `stream` (a torch.cuda.Stream); returns a torch event recorded behind it."""
    import torch
    cycles = int(ms * cycles_per_ms())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        ev = torch.cuda.Event()
        ev.record()
    return ev


class Hold:
    """One hold and the window a case places its calls in."""

    def __init__(self, stream, ms=HOLD_MS):
        self.stream, self.ms = stream, ms
        cycles_per_ms()                                     # (not inside the window)
        self.t0 = time.perf_counter()
        self.event = hold(stream, ms)

    def pending(self):
        return not self.event.query()

    def lap(self, step):
        """print how far into the window `step` returned (which call of a window took the time, when one is too long)"""
        print(f"stream_hold: {step} returned {(time.perf_counter() - self.t0) * 1e3:.3f} ms into the hold")

    def must_be_pending(self, case):
        """Right after the last call placed in the window: the hold still holds, or the case has shown nothing and fails."""
        window = (time.perf_counter() - self.t0) * 1e3
        pending = self.pending()
        WINDOWS.append((case, window))
        print(f"stream_hold: {case}: window {window:.3f} ms of a {self.ms:.0f} ms hold, {'still pending' if pending else 'ALREADY OVER'}")
        assert pending, (f"{case}: the hold of {self.ms:.0f} ms had already ended {window:.3f} ms after it was queued, before the calls that race "
                         f"with it were all submitted: the case shows nothing")

    def release(self):
        """Wait for the hold to run out (bounded: it is a spin of self.ms)."""
        self.event.synchronize()


class Ballast:
    """HIP streams that exist only to occupy hardware queues. A case that holds torch's default stream cannot take another stream to hold; what
    it can move is the session's: the runtime deals a new stream the next queue (or the least used one), so a session opened after one more
    ballast stream was made gets other queues than the session before it. Made through the HIP runtime this process has already loaded."""

    def __init__(self):
        self.streams, self.runtime = [], None

    def add(self):
        import ctypes
        if self.runtime is None:
            with open("/proc/self/maps") as maps:
                paths = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
            if not paths:
                return
            self.runtime = ctypes.CDLL(paths[0])
        stream = ctypes.c_void_p()
        if self.runtime.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0:      # hipStreamNonBlocking
            self.streams.append(stream)

    def free(self):
        for stream in self.streams:
            self.runtime.hipStreamDestroy(stream)
        self.streams = []


def independent(case, attempt):
    """The control of a case. attempt(side) -- side: a fresh torch side stream -- queues its hold, runs the operation that must not be
    ordered behind it, and returns (ok, value): ok = that operation completed while the hold was pending. On ok the case goes on with
    `value`; otherwise the hold is left to run out and another stream is tried, MAX_ATTEMPTS in all. Streams tried are kept alive, and
    a ballast stream is added after each attempt that failed, so that the runtime does not deal the same queues out again (an attempt
    that opens a session of its own has closed it by then)."""
    import torch
    tried, ballast = [], Ballast()
    try:
        for k in range(MAX_ATTEMPTS):
            side = torch.cuda.Stream(device="cuda:0")
            tried.append(side)
            ok, value = attempt(side)
            if ok:
                if k:
                    print(f"stream_hold: {case}: the control held on attempt {k + 1}")
                return value
            torch.cuda.synchronize()
            ballast.add()
    finally:
        ballast.free()
    pytest.fail(f"{case}: inconclusive -- in {MAX_ATTEMPTS} attempts the operation that should be independent of the held stream did not "
                f"complete while the hold was pending (streams sharing a hardware queue)")
