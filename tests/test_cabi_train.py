"""The raw-parameter step's entries (include/gsr_hip_train.h: gsr_adam_act_step, gsr_activate) on a machine without a GPU: every refusal the
header lists returns GSR_E_INVALID with a message naming the entry.  (That the header, the library and the binding agree is
tests/test_cabi.py's, for every header.)  The calls are made with fake pointers in a child process that sees no GPU (tests/cabi_child.py);
`python test_cabi_train.py` is that child."""
import sys

import pytest

import cabi_child
from cabi_args import FAKE

ENTRIES = ("gsr_adam_act_step", "gsr_activate")

# ------------------------------------------------------------------------------------------------- the refusals
# One well-formed call per entry: 1000 floats, three segments (plain, sigmoid, normalize), a compact activated buffer of 600.
N, N_ACT = 1000, 600
_SEGS = ((0, 400, 1e-3, 0.0, 0, 0, 0, 0), (400, 600, 1e-3, 0.0, 0, 0, 1, 0), (600, 1000, 1e-3, 0.0, 0, 0, 3, 200))


def _with(i, **kw):
    """_SEGS with fields of segment i replaced."""
    names = ("begin", "end", "lr", "lr2", "period", "split", "kind", "act_begin")
    segs = [list(s) for s in _SEGS]
    for k, v in kw.items():
        segs[i][names.index(k)] = v
    return tuple(tuple(s) for s in segs)


STEP_ARGS = ("raw", "grad", "exp_avg", "exp_avg_sq", "act", "n", "n_act", "segments", "num_segments", "beta1", "beta2", "eps", "step", "range_begin",
             "range_end", "stream")
ACTIVATE_ARGS = ("raw", "act", "n", "n_act", "segments", "num_segments", "stream")
BASE = dict(raw=FAKE, grad=FAKE, exp_avg=FAKE, exp_avg_sq=FAKE, act=FAKE, n=N, n_act=N_ACT, segments=_SEGS, num_segments=3, beta1=0.9, beta2=0.999,
            eps=1e-15, step=1, range_begin=0, range_end=N, stream=None)

# what both entries refuse (the header's list), as changes to the well-formed call
SHARED = {
    "null:raw": dict(raw=None), "misaligned:raw": dict(raw=FAKE + 4),
    "null:segments": dict(segments=None), "num_segments=0": dict(num_segments=0), "num_segments>16": dict(num_segments=17),
    "segments-stop-short-of-n": dict(segments=_with(2, end=996)),
    "segments-out-of-order": dict(segments=_with(1, begin=396)),
    "segment-split>period": dict(segments=_with(0, period=48, split=49)),
    "null:act-with-an-activated-segment": dict(act=None),
    "misaligned:act": dict(act=FAKE + 4),
    "unknown-kind": dict(segments=_with(1, kind=4)),
    "unknown-flag-bit": dict(segments=_with(1, kind=1 | 0x200)),
    "activated-begin-not-a-multiple-of-4": dict(segments=((0, 398, 1e-3, 0.0, 0, 0, 0, 0), (398, 600, 1e-3, 0.0, 0, 0, 1, 0),
                                                          (600, 1000, 1e-3, 0.0, 0, 0, 3, 204)), n_act=608),
    "act_begin-not-a-multiple-of-4": dict(segments=_with(1, act_begin=2)),
    "normalize4-length-not-a-multiple-of-4": dict(segments=((0, 400, 1e-3, 0.0, 0, 0, 0, 0), (400, 598, 1e-3, 0.0, 0, 0, 3, 0),
                                                            (598, 1000, 1e-3, 0.0, 0, 0, 0, 0))),
    "segment-past-n_act": dict(n_act=599),
    "act_begin-past-n_act": dict(segments=_with(2, act_begin=1 << 40)),
}
STEP_ONLY = {
    "null:grad": dict(grad=None), "null:exp_avg": dict(exp_avg=None), "null:exp_avg_sq": dict(exp_avg_sq=None),
    "misaligned:grad": dict(grad=FAKE + 4), "misaligned:exp_avg": dict(exp_avg=FAKE + 4), "misaligned:exp_avg_sq": dict(exp_avg_sq=FAKE + 4),
    "step=0": dict(step=0), "step<0": dict(step=-1),
    "range_begin-not-a-multiple-of-4": dict(range_begin=2), "range_end>n": dict(range_end=1004), "range_begin>range_end": dict(range_begin=8, range_end=4),
    "range_end-inside-not-a-multiple-of-4": dict(range_end=998),
}
# calls that must NOT be refused
OK = {
    "well-formed": {}, "frozen-flag": dict(segments=_with(2, kind=3 | 0x100)),
    "no-activated-segment-needs-no-act": dict(act=None, n_act=0, segments=((0, 1000, 1e-3, 0.0, 0, 0, 0, 0),), num_segments=1),
}
NOOP = {"n=0": dict(n=0, raw=None, segments=None)}
STEP_NOOP = {"empty-range": dict(range_begin=400, range_end=400)}


def cases():
    """[(entry, case id, expectation)]: "refused", "accepted" (anything but a refusal: without a device the launch fails) or "noop" (returns 0)."""
    out = []
    for entry in ENTRIES:
        step = entry == "gsr_adam_act_step"
        out += [(entry, k, "accepted") for k in OK] + [(entry, k, "noop") for k in NOOP]
        out += [(entry, k, "refused") for k in SHARED]
        if step:
            out += [(entry, k, "refused") for k in STEP_ONLY] + [(entry, k, "noop") for k in STEP_NOOP]
    return out


def _changes(case):
    for table in (OK, NOOP, SHARED, STEP_ONLY, STEP_NOOP):
        if case in table:
            return table[case]
    raise KeyError(case)


_keep = []


def _call(gsr, entry, case):
    args = dict(BASE, **_changes(case))
    if args["segments"] is not None:
        arr = (gsr.ActSegment * 17)()
        for i, seg in enumerate(args["segments"]):
            arr[i] = gsr.ActSegment(*seg)
        _keep.append(arr)
        args["segments"] = arr
    names = STEP_ARGS if entry == "gsr_adam_act_step" else ACTIVATE_ARGS
    return getattr(gsr.lib, entry)(*[args[k] for k in names])


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    return cabi_child.run(__file__)


@pytest.mark.parametrize("entry, case, expect", cases(), ids=lambda v: v)
def test_refusal(outcomes, entry, case, expect):
    cabi_child.check(outcomes, entry, case, expect)


if __name__ == "__main__":
    sys.exit(cabi_child.serve([c[:2] for c in cases()], _call))
