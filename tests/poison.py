"""Poisoned allocations: a test harness that shows whether any result depends on what an uninitialised buffer held.

Every output plane, workspace and scratch region of the package is allocated in Python with `torch.empty` (or one of its siblings) and
handed to the library as a pointer.  In a fresh process those bytes are, in practice, zero; in training they are whatever the caching
allocator returns from the step before.  `poisoned(pattern)` replaces every allocation form the package uses so that each tensor of the
given device type comes back filled byte-wise with `pattern`:

    0x00   float32 0          int32 0           the baseline (what a fresh process sees)
    0xFF   float32 NaN        int32 -1          every flag set, every counter at its maximum
    0x01   float32 2.4e-38    int32 16843009    finite garbage that survives a NaN check

The fill goes through a uint8 view of the tensor on the current stream, so it is ordered in front of the kernel that takes the buffer.
`torch.zeros`, `torch.full` and their `new_` / `_like` forms are left alone.  Not a conftest: tests import it.

The compiled binding (csrc/gsr_torch_binding.cpp) allocates in C++, out of this harness's reach.  The wrappers read `_gsr.PYBIND` on every
call, and both bindings drive the same HIP library, so `ctypes_binding()` forces the calls of a test onto the ctypes path: within it
`_gsr.PYBIND is None` holds whether or not the compiled binding is built, and no test has to skip.
"""
import contextlib

import torch

PATTERNS = (0x00, 0xFF, 0x01)          # 0x00 first: a test runs the baseline before the patterns that may send an index astray

# the allocation forms the package uses (tests/test_poison_host.py scans the package for any other): (owner, attribute)
PATCHED = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty"))
PATCHED_NAMES = frozenset(("torch.empty", "torch.empty_like", "torch.empty_strided", ".new_empty"))


class Poison:
    """What `poisoned` yields: the number of tensors filled and their bytes."""

    def __init__(self, pattern, device_type):
        self.pattern, self.device_type = int(pattern), device_type
        self.count = 0
        self.bytes = 0

    def fill(self, t):
        if isinstance(t, torch.Tensor) and t.device.type == self.device_type and t.numel() > 0:
            # fresh from an allocator: its storage is its own.  A dense tensor is filled through a uint8 view of itself; anything else
            # (empty_strided with gaps) through a uint8 view of its whole storage
            if t.is_contiguous():
                t.view(torch.uint8).fill_(self.pattern)
                nbytes = t.numel() * t.element_size()
            else:
                st = t.untyped_storage()
                nbytes = st.nbytes()
                torch.empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (nbytes,), (1,)).fill_(self.pattern)
            self.count += 1
            self.bytes += nbytes
        return t


def _wrap(orig, state):
    def alloc(*args, **kwargs):
        return state.fill(orig(*args, **kwargs))
    alloc.__wrapped__ = orig
    return alloc


@contextlib.contextmanager
def poisoned(pattern, device_type="cuda"):
    """Within the scope, every tensor of `device_type` with numel() > 0 that `torch.empty`, `torch.empty_like`, `torch.empty_strided` or
    `Tensor.new_empty` returns is filled byte-wise with `pattern`.  Yields the counter; restores the originals on exit, also after an
    exception."""
    if not 0 <= int(pattern) <= 0xFF:
        raise ValueError("pattern is one byte")
    state = Poison(pattern, device_type)
    # (an attribute the owner inherits, as Tensor.new_empty from its base class, is restored by deleting the override: the owner's own
    # dictionary is left as it was)
    saved = [(owner, name, getattr(owner, name), name in vars(owner)) for owner, name in PATCHED]
    try:
        for owner, name, orig, own in saved:
            setattr(owner, name, _wrap(orig, state))
        yield state
    finally:
        for owner, name, orig, own in saved:
            if own:
                setattr(owner, name, orig)
            elif name in vars(owner):
                delattr(owner, name)


@contextlib.contextmanager
def ctypes_binding():
    """Calls made in the scope take the ctypes marshaling of _gsr.py (whose allocations are Python's) also where the compiled binding is
    loaded.  The wrappers consult `_gsr.PYBIND` per call, so nothing of the package changes."""
    import _gsr
    saved = _gsr.PYBIND
    _gsr.PYBIND = None
    try:
        yield
    finally:
        _gsr.PYBIND = saved


def u32(a):
    """Bit pattern of an array for exact comparison (NaNs compare by their bits): uint32 words for 4-byte elements, else bytes."""
    import numpy as np
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 4:
        return a.view(np.uint32)
    if a.dtype.itemsize == 8:
        return a.view(np.uint32)
    return a.view(np.uint8)
