"""The two timers of the decoder's bench tools (bench_generate.py, bench_beam.py, bench_decode_controls.py, bench_score.py)."""
import time

import torch


def replayed_us(body, n, reps, warm=3):
    """us of device time per call of body(j): after `warm` calls, body(0) .. body(n - 1) are captured into one graph on the current
    stream and the graph is replayed.  Returns (the best of `reps` replays, max / min over them)."""
    for j in range(warm):
        body(j)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for j in range(n):
            body(j)
    g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1) / n)
    return min(ts), max(ts) / min(ts)


def wall_ms(fn, reps, calls=1, warm=1):
    """ms of wall-clock time per call of fn(): after `warm` calls, `calls` of them between two synchronisations.  Returns (the best of
    `reps` such timings, max / min over them)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0) / calls)
    return min(ts), max(ts) / min(ts)
