"""Timing scaffold of tools/barlow_bench.py and tools/vicreg_bench.py: device events around a run of
calls, medians, and the interleaved rounds baseline, new, baseline."""
from __future__ import annotations

import statistics

import torch


def timed(fn, iters):
    """ms per call of ``iters`` calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def med(xs):
    return statistics.median(xs)


def interleaved(base, new, rounds, iters):
    """-> medians (base series 1, base series 2, new) and new's range."""
    for _ in range(3):
        base()
        new()
    ta, tn, tb = [], [], []
    for _ in range(rounds):
        ta.append(timed(base, iters))
        tn.append(timed(new, iters))
        tb.append(timed(base, iters))
    return med(ta), med(tb), med(tn), min(tn), max(tn)
