"""What the input stages' measuring tools (bench_quality.py, bench_appearance.py, bench_jpeg.py, bench_clahe.py) share: the timed
window, the alternating loop over variants, and the writer that keeps a profile's hand-written tail."""
import os

import torch


def window(fn, inner):
    """ms per call over `inner` back-to-back calls, between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def alternate(fns, reps, inner, warmup=5):
    """fns: name -> callable.  `warmup` calls of each (code objects, allocator), then `reps` rounds of one `window` per variant —
    alternating: other people's work shares the machine.  -> name -> [ms per call] * reps."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(window(fn, inner))
    return times


def write_profile(path, lines, marker="## Reading the numbers"):
    """Write and print `lines`; what an existing file holds from `marker` on — written by hand below the tables — is kept."""
    text = "\n".join(lines)
    if os.path.isfile(path):
        old = open(path).read()
        if marker in old:
            text += old[old.index(marker):]
    with open(path, "w") as f:
        f.write(text)
    print(text)
