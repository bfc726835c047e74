"""The raw-parameter step's entries (include/gsr_hip_train.h: gsr_adam_act_step, gsr_activate) on a machine without a GPU: the header parses
as include/gsr_hip.h does, the library exports both, the ctypes prototypes and the descriptor struct match, and every refusal the header
lists returns GSR_E_INVALID with a message naming the entry.  The calls are made with fake pointers in ONE child process that hides every
GPU and asks the HIP runtime for the device count first (tests/cabi_args.py's guard, by import); with a device still visible nothing is
called.  `python test_cabi_train.py` is that child."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

import cabi_args
from cabi_args import FAKE, GSR_E_INVALID

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "gsr_hip_train.h")
ENTRIES = ("gsr_adam_act_step", "gsr_activate")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _protos():
    """[(entry, argument text)] with the regex of tests/test_cabi.py."""
    return re.findall(r"(?:int|size_t|const char\*)\s+(gsr_\w+)\s*\(([^;]*?)\)\s*;", _source(), flags=re.S)


def test_header_declares_the_two_entries_and_includes_the_main_header():
    assert sorted(n for n, _ in _protos()) == sorted(ENTRIES)
    assert re.search(r'#include "gsr_hip\.h"', open(HEADER).read())
    assert "GSR_ABI_VERSION" not in _source()            # the version is the main header's, and stays


def test_library_exports_both_and_the_lists_are_disjoint(hip_lib_built):
    import _gsr
    raw = ctypes.CDLL(_gsr.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(raw, n), f"{n} declared in gsr_hip_train.h but not exported by libgsr_hip.so"
    assert sorted(_gsr.EXPORTED_TRAIN) == sorted(ENTRIES)
    assert not set(_gsr.EXPORTED_TRAIN) & set(_gsr.EXPORTED)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr_hip.h")).read(), flags=re.S)
    for n in ENTRIES:
        assert n not in main
    assert _gsr.lib.gsr_version() == _gsr.GSR_ABI_VERSION == 102


def test_ctypes_signatures_and_struct_match_header(hip_lib_built):
    import _gsr

    def ctype(arg):
        arg = arg.strip()
        if arg.startswith("const gsr_act_segment*"):
            return ctypes.POINTER(_gsr.ActSegment)
        if "*" in arg:
            return ctypes.c_void_p
        for pre, t in (("float", ctypes.c_float), ("uint32_t", ctypes.c_uint32), ("uint64_t", ctypes.c_uint64), ("size_t", ctypes.c_size_t),
                       ("int", ctypes.c_int)):
            if arg.startswith(pre):
                return t
        raise ValueError(arg)

    for name, args in _protos():
        fn = getattr(_gsr.lib, name)
        assert [ctype(a) for a in args.split(",")] == list(fn.argtypes), name
        assert fn.restype is ctypes.c_int
    body = re.search(r"typedef struct \{([^}]*)\}\s*gsr_act_segment;", _source(), flags=re.S).group(1)
    types = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            t, names = decl.split(None, 1)
            fields += [(n.strip(), types[t]) for n in names.split(",")]
    assert fields == list(_gsr.ActSegment._fields_)
    src = _source()
    for k, v in (("NONE", _gsr.GSR_ACT_NONE), ("SIGMOID", _gsr.GSR_ACT_SIGMOID), ("EXP", _gsr.GSR_ACT_EXP), ("NORMALIZE4", _gsr.GSR_ACT_NORMALIZE4),
                 ("FROZEN", _gsr.GSR_ACT_FROZEN)):
        assert int(re.search(r"#define GSR_ACT_%s (\w+)" % k, src).group(1), 0) == v


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


def _child():
    os.environ.update(cabi_args.HIDE_GPUS)
    sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-reflection_amd"))
    import _gsr
    n = cabi_args._visible_devices()
    print(json.dumps({"devices": n}), flush=True)
    if n != 0:
        return 0
    keep = []
    for entry, case, _ in cases():
        args = dict(BASE, **_changes(case))
        if args["segments"] is not None:
            arr = (_gsr.ActSegment * 17)()
            for i, s in enumerate(args["segments"]):
                arr[i] = _gsr.ActSegment(*s)
            keep.append(arr)
            args["segments"] = arr
        names = STEP_ARGS if entry == "gsr_adam_act_step" else ACTIVATE_ARGS
        print(json.dumps({"begin": [entry, case]}), flush=True)
        rc = getattr(_gsr.lib, entry)(*[args[k] for k in names])
        msg = _gsr.lib.gsr_last_error()
        print(json.dumps({"done": [entry, case], "rc": int(rc), "msg": msg.decode(errors="replace") if msg else ""}), flush=True)
    return 0


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    env = dict(os.environ, **cabi_args.HIDE_GPUS)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    done, begun = {}, None
    for line in p.stdout.splitlines():
        if not line.startswith("{"):
            continue
        rec = json.loads(line)
        if "devices" in rec and rec["devices"] != 0:
            return None
        if "begin" in rec:
            begun = tuple(rec["begin"])
        elif "done" in rec:
            done[tuple(rec["done"])] = rec
            begun = None
    assert p.returncode == 0 and begun is None, f"the child ended in {begun} (exit {p.returncode}):\n{p.stderr[-2000:]}"
    return done


@pytest.mark.parametrize("entry, case, expect", cases(), ids=lambda v: v)
def test_refusal(outcomes, entry, case, expect):
    if outcomes is None:
        pytest.skip("a GPU is still visible to the child process although the visible-devices variables hide them: nothing is called")
    got = outcomes.get((entry, case))
    assert got is not None, "the child never reached this call"
    if expect == "refused":
        assert got["rc"] == GSR_E_INVALID, (entry, case, got)
        assert got["msg"].startswith(entry), (entry, case, got["msg"])
    elif expect == "noop":
        assert got["rc"] == 0, (entry, case, got)
    else:
        assert got["rc"] != GSR_E_INVALID, (entry, case, got)


if __name__ == "__main__":
    sys.exit(_child())
