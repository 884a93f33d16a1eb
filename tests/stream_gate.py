"""A gate that makes the order of work on two streams observable (tests/test_gpu_streams.py).

``gate(stream, seconds)`` parks bounded busy work at the head of ``stream``; everything enqueued on that stream afterwards -- and
everything that correctly waits for it on another stream -- cannot start before the gate ends.  A reader on another stream that does
NOT wait runs at once and sees what was in memory before.  ``calibrate`` shows, on the test's own torch memory, that this machine does
run such a reader concurrently; without that a gated case has no power.

The gate is sized at run time (``gate_length``): at least ``MIN_FACTOR`` times the host time the case needed to enqueue its calls in an
un-gated pass, never longer than ``MAX_GATE_S``.  Those two are a condition, not a measurement: a case asserts ``still_closed`` after
its last enqueue, and fails if the gate had already ended."""
import pytest
import torch

MAX_GATE_S = 0.5
MIN_FACTOR = 20
FLOOR_S = 0.03           # shorter gates are not worth the risk of a late host: 30 ms is far above any timer's noise
CALIBRATION_GATE_S = 0.05
MAX_CANDIDATES = 8       # (processes here open a few hardware queues: of eight fresh streams some pair runs side by side)

_cycles_per_second = {}


def cycles_per_second(device) -> float:
    """how many ``torch.cuda._sleep`` cycles last a second on ``device``: measured once, with a spin long enough to time"""
    device = torch.device(device)
    if device not in _cycles_per_second:
        with torch.cuda.device(device):
            torch.cuda._sleep(1000)  # (loads the kernel)
            cycles, ms = 2_000_000, 0.0
            for _ in range(6):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                torch.cuda._sleep(cycles)
                b.record()
                torch.cuda.synchronize()
                ms = a.elapsed_time(b)
                if ms >= 5.0:
                    break
                cycles *= 8
            if ms < 5.0:
                pytest.fail(f"torch.cuda._sleep({cycles}) lasted {ms:.3f} ms: cannot size a gate with it")
            _cycles_per_second[device] = cycles / (ms * 1e-3)
    return _cycles_per_second[device]


def gate_length(enqueue_s: float) -> float:
    """the gate of a case whose calls took ``enqueue_s`` of host time to enqueue un-gated"""
    need = MIN_FACTOR * enqueue_s
    if need > MAX_GATE_S:
        pytest.fail(f"enqueueing took {enqueue_s * 1e3:.2f} ms un-gated: a gate of {MIN_FACTOR} times that exceeds {MAX_GATE_S} s")
    return max(need, FLOOR_S)


def gate(stream, seconds: float = MAX_GATE_S):
    """busy work of ``seconds`` (at most MAX_GATE_S) on ``stream``; returns an event recorded behind it"""
    seconds = min(float(seconds), MAX_GATE_S)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(seconds * cycles_per_second(stream.device)))
        done = torch.cuda.Event()
        done.record(stream)
    return done


def still_closed(done) -> bool:
    """has the gate's work not finished yet?"""
    return not done.query()


def calibrate(gated, candidates):
    """(index, stream) of the first of ``candidates`` on which a reader that does not wait for ``gated`` sees the OLD value of memory
    that ``gated`` overwrites behind a gate: the two streams run concurrently here.  None does: the module fails."""
    device = gated.device
    tried = []
    for i, cand in enumerate(candidates[:MAX_CANDIDATES]):
        x = torch.zeros(4096, device=device)
        y = torch.full((4096,), -1.0, device=device)
        torch.cuda.synchronize(device)
        done = gate(gated, CALIBRATION_GATE_S)
        with torch.cuda.stream(gated):
            x.fill_(1.0)
        with torch.cuda.stream(cand):
            y.copy_(x)  # no wait for `gated`
        closed = still_closed(done)
        torch.cuda.synchronize(device)
        old = bool((y == 0).all())
        assert bool((x == 1).all())
        tried.append((i, closed, old, float(y[0])))
        if closed and old:
            print(f"[stream_gate] calibration: candidate {i} of {len(candidates)} runs beside the gated stream "
                  f"(an unordered reader saw the old value; gate {CALIBRATION_GATE_S * 1e3:.0f} ms)")
            return i, cand
    pytest.fail(f"no candidate stream ran concurrently with the gated one: (candidate, gate still closed, reader saw the old value, y[0]) = {tried}")
