"""What the learner-path timing tools share (time_record.py, time_record_obs.py, time_record_logp.py, time_backward.py,
time_backward_samples.py): the clock -- HIP events around alternating blocks, or around single calls --, the median (min-max) column
and the parent process that runs every shape or dtype in a child of its own under a time limit.  Importing it puts the repository
root on sys.path, so a tool run as `python tools/<tool>.py` finds the package."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def fmt(ts, digits):
    """median (min-max) of a series, `digits` decimals."""
    return f"{statistics.median(ts):{digits + 6}.{digits}f} ({min(ts):.{digits}f}-{max(ts):.{digits}f})"


def alternate(modes, reps, n, after=None):
    """{name: [µs per step]} of `reps` rounds over modes = [(name, fn)], a block fn(n) of every mode per round, after one warm-up
    round that is dropped: HIP events around each block, the device idle before the first and the host waiting for the second.
    after: {name: callback}, called behind every block of that mode (the warm-up round's too)."""
    import torch
    times = {name: [] for name, _ in modes}
    for rep in range(reps + 1):   # (the first round is the warm-up)
        for name, fn in modes:
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(n)
            b.record()
            b.synchronize()
            if rep > 0:
                times[name].append(a.elapsed_time(b) * 1000.0 / n)
            if after and name in after:
                after[name]()
    return times


def repeat_ms(fn, reps, warmup):
    """[ms] of `reps` calls of fn(), HIP events around each, after `warmup` calls and one synchronisation."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def run_children(script, n_children, passthrough_args, limit, label):
    """`script --child i <passthrough_args>` for i = 0 .. n_children - 1, each a process of its own that may take `limit` seconds
    (running out of them counts as status 124).  After a child that ends with another status than 0 one line says so -- label(i)
    names the child -- and nothing more is started.  Returns that status, or 0."""
    for i in range(n_children):
        cmd = [sys.executable, os.path.abspath(script), "--child", str(i), *passthrough_args]
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"{label(i)} ended with status {rc}" + (": nothing more is started" if n_children > 1 else ""), flush=True)
            return rc
    return 0
