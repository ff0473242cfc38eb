"""GPU timing with events on the current stream.  No imports from this package: renderer, fused and roofline all use it."""
import numpy as np
import torch


def _time_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return float(np.mean([a.elapsed_time(b) for a, b in evs]))


class _Stamps:
    """Optional per-stage GPU timing with events on the current stream."""

    def __init__(self, sink):
        self.sink = sink
        self.ev = []

    def mark(self, name):
        if self.sink is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.ev.append((name, e))

    def done(self):
        if self.sink is not None and self.ev:
            torch.cuda.synchronize()
            for (n0, e0), (n1, e1) in zip(self.ev[:-1], self.ev[1:]):
                self.sink.setdefault(n1, []).append(e0.elapsed_time(e1))
