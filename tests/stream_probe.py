"""Tools for the stream-ordering tests (tests/test_gpu_streams.py).  Nothing here touches the GPU at import.

On one stream everything serialises, so a kernel enqueued on the wrong stream, a missing event between two streams or a cached device
tensor built on another stream cannot be seen.  The arrangement that shows them:

    late_inputs(s, arrays)   device tensors that hold poison (NaN / -1) until a delay on stream `s` has run out; only then do the real
                             values arrive, by copies enqueued on `s` behind the delay.  Work that is ordered behind `s` reads the real
                             values; anything that is not reads the poison, and a NaN fails at any tolerance.
    fetch(s, tensors)        the results, copied to pinned host memory on `s` and read after synchronising `s` ALONE: work that ran on
                             another stream without an event back to `s` is not waited for.

The delay is `torch.cuda._sleep(cycles)`: a kernel that spins for a number of device clock ticks.  Ticks per millisecond are measured once
per process with two events (no figure is assumed); 50 ms only has to outlast the host's enqueueing of the calls placed behind it.  Whether
it does on the machine at hand is shown by the negative control of tests/test_gpu_streams.py, not assumed.

Not a conftest: tests import it."""
import numpy as np

DEFAULT_DELAY_MS = 50.0
_cycles_per_ms = None


def cycles_per_ms():
    """Ticks of `torch.cuda._sleep` per millisecond on the current device, measured on first use: the sleep is lengthened tenfold until it
    takes at least 2 ms between two events, then scaled."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch
        torch.cuda._sleep(1000)                 # (loads the kernel)
        torch.cuda.synchronize()
        cycles = 100_000
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 2.0 or cycles >= 10 ** 11:
                break
            cycles *= 10
        if not ms > 0.0:
            raise RuntimeError("stream_probe: torch.cuda._sleep(%d) took no measurable time" % cycles)
        _cycles_per_ms = cycles / ms
    return _cycles_per_ms


def delay(stream, ms=DEFAULT_DELAY_MS):
    """Holds `stream` back by about `ms` milliseconds of device time.  The host does not wait."""
    import torch
    cycles = int(cycles_per_ms() * ms)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def _poison(t):
    import torch
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    elif t.dtype == torch.bool:
        t.fill_(True)
    else:
        t.fill_(-1)                             # (every bit set: 255 for uint8)
    return t


def late_inputs(stream, tensors, ms=DEFAULT_DELAY_MS):
    """tensors: a dict (or list / tuple) of numpy arrays or CPU tensors; anything else (numbers, None) passes through.  Returns the same
    structure with each array as a device tensor allocated on `stream` that holds NaN (floats), -1 (integers) or True (bool) until `ms`
    of delay on `stream` have passed and the copy of the real values, enqueued behind the delay, has run."""
    import torch
    is_dict = isinstance(tensors, dict)
    keys = list(tensors.keys()) if is_dict else list(range(len(tensors)))
    out, pending = {}, []
    with torch.cuda.stream(stream):
        for k in keys:
            v = tensors[k]
            if isinstance(v, np.ndarray):
                v = torch.from_numpy(np.ascontiguousarray(v))
            if not isinstance(v, torch.Tensor):
                out[k] = v
                continue
            host = v.detach().contiguous().pin_memory()
            dev = _poison(torch.empty(host.shape, dtype=host.dtype, device="cuda"))
            out[k] = dev
            pending.append((dev, host))
    stream.synchronize()                        # the poison is in memory before anybody can look
    delay(stream, ms)
    with torch.cuda.stream(stream):
        for dev, host in pending:
            dev.copy_(host, non_blocking=True)
    return out if is_dict else type(tensors)(out[k] for k in keys)


def fetch(stream, tensors):
    """tensors: a dict (or list / tuple) of device tensors (None passes through).  Copies them to pinned host memory on `stream`,
    synchronises that stream only and returns numpy arrays in the same structure."""
    import torch
    is_dict = isinstance(tensors, dict)
    keys = list(tensors.keys()) if is_dict else list(range(len(tensors)))
    hosts = {}
    with torch.cuda.stream(stream):
        for k in keys:
            t = tensors[k]
            if t is None:
                hosts[k] = None
                continue
            t = t.detach().contiguous()
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            hosts[k] = h
    stream.synchronize()
    out = {k: (None if h is None else h.numpy().copy()) for k, h in hosts.items()}
    return out if is_dict else type(tensors)(out[k] for k in keys)


# ------------------------------------------------------------------------------------------------------------ comparators
def same_bits(a, b):
    """Same shape, same dtype, same bytes.  NaN equals NaN only where the bit patterns agree; -0.0 differs from 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8)))


def deviation(a, b):
    """max|a - b| / max|b| in float64 (max|a - b| itself where b is all zero); inf for a shape mismatch or a non-finite element of `a`."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.isfinite(a).all():
        return float("inf")
    if a.size == 0:
        return 0.0
    d = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    den = float(np.abs(b.astype(np.float64)).max())
    if not np.isfinite(d) or not np.isfinite(den):
        return float("inf")
    return d / den if den > 0 else d


def close_to_serial(a, b, frac):
    """max|a - b| <= frac * max|b| with `a` finite everywhere and of b's shape (a NaN in `a` fails, also where `b` has one too)."""
    return deviation(a, b) <= frac
