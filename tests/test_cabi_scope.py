"""The env-scope entries (include/gsr_hip_scope.h: gsr_env_scope_scratch_floats, gsr_env_scope_forward, gsr_env_scope_backward) on a machine
without a GPU: the header parses as include/gsr_hip.h does, the library exports the three, the ctypes prototypes match, and every refusal
the header lists returns GSR_E_INVALID with a message naming the entry.  The calls are made with fake pointers in ONE child process that
hides every GPU and asks the HIP runtime for the device count first (tests/cabi_args.py's guard, by import); with a device still visible
nothing is called.  `python test_cabi_scope.py` is that child."""
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
HEADER = os.path.join(ROOT, "include", "gsr_hip_scope.h")
ENTRIES = ("gsr_env_scope_scratch_floats", "gsr_env_scope_forward", "gsr_env_scope_backward")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _protos():
    """[(return type, entry, argument text)] with the regex of tests/test_cabi.py."""
    return re.findall(r"(int|size_t|const char\*)\s+(gsr_\w+)\s*\(([^;]*?)\)\s*;", _source(), flags=re.S)


def test_header_declares_the_three_entries_and_includes_the_main_header():
    assert sorted(n for _, n, _ in _protos()) == sorted(ENTRIES)
    assert re.search(r'#include "gsr_hip\.h"', open(HEADER).read())
    assert "GSR_ABI_VERSION" not in _source()            # the version is the main header's, and stays


def test_library_exports_them_and_the_lists_are_disjoint(hip_lib_built):
    import _gsr
    raw = ctypes.CDLL(_gsr.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(raw, n), f"{n} declared in gsr_hip_scope.h but not exported by libgsr_hip.so"
    assert sorted(_gsr.EXPORTED_SCOPE) == sorted(ENTRIES)
    assert not set(_gsr.EXPORTED_SCOPE) & set(_gsr.EXPORTED)
    assert not set(_gsr.EXPORTED_SCOPE) & set(_gsr.EXPORTED_TRAIN)
    for other in ("gsr_hip.h", "gsr_hip_train.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        for n in ENTRIES:
            assert n not in text, (n, other)
    assert _gsr.lib.gsr_version() == _gsr.GSR_ABI_VERSION == 102


def test_ctypes_signatures_match_header(hip_lib_built):
    import _gsr

    def ctype(arg):
        arg = arg.strip()
        if "*" in arg:
            return ctypes.c_void_p
        for pre, t in (("float", ctypes.c_float), ("size_t", ctypes.c_size_t), ("int", ctypes.c_int)):
            if arg.startswith(pre):
                return t
        raise ValueError(arg)

    for ret, name, args in _protos():
        fn = getattr(_gsr.lib, name)
        want = [] if args.strip() == "void" else [ctype(a) for a in args.split(",")]
        assert want == list(fn.argtypes), name
        assert fn.restype is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int), name


def test_python_layer_asks_for_a_rebuild_when_the_entries_are_missing(hip_lib_built, monkeypatch):
    from utils import loss_utils
    real = loss_utils.lib

    class Old:
        """A library built before the env-scope pass: everything but the three entries."""
        def __getattr__(self, name):
            if name in ENTRIES:
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(loss_utils, "lib", Old())
    for call in (lambda: loss_utils.env_scope_masks(None, (0, 0, 0), 1.0), lambda: loss_utils.refl_scope_loss(None, None, (0, 0, 0), 1.0)):
        with pytest.raises(ImportError, match="rebuild"):
            call()


# ------------------------------------------------------------------------------------------------- the refusals
FORWARD_ARGS = ("P", "means3D", "refl", "cx", "cy", "cz", "radius2", "inside", "outside", "sums", "scratch", "stream")
BACKWARD_ARGS = ("P", "outside", "sums", "g_loss", "grad_refl", "accumulate", "stream")
BASE = {
    "gsr_env_scope_forward": dict(P=1000, means3D=FAKE, refl=FAKE, cx=0.3, cy=-1.2, cz=2.5, radius2=2.89, inside=FAKE, outside=FAKE, sums=FAKE,
                                  scratch=FAKE, stream=None),
    "gsr_env_scope_backward": dict(P=1000, outside=FAKE, sums=FAKE, g_loss=FAKE, grad_refl=FAKE, accumulate=0, stream=None),
}
INF, NAN = float("inf"), float("nan")
MASKS_ONLY = dict(refl=None, sums=None, scratch=None)
REFUSED = {
    "gsr_env_scope_forward": {
        "neg:P": dict(P=-1), "null:means3D": dict(means3D=None),
        "refl-without-outside": dict(outside=None), "refl-without-sums": dict(sums=None), "refl-without-scratch": dict(scratch=None),
        "nothing-to-do": dict(MASKS_ONLY, inside=None, outside=None),
        "cx=inf": dict(cx=INF), "cy=-inf": dict(cy=-INF), "cz=nan": dict(cz=NAN), "cx=nan-masks-only": dict(MASKS_ONLY, cx=NAN),
        "radius2=inf": dict(radius2=INF), "radius2=nan": dict(radius2=NAN), "radius2<0": dict(radius2=-1e-6),
        "radius2=inf-with-P=0": dict(P=0, radius2=INF),
    },
    "gsr_env_scope_backward": {
        "neg:P": dict(P=-1), "null:outside": dict(outside=None), "null:sums": dict(sums=None), "null:g_loss": dict(g_loss=None),
        "null:grad_refl": dict(grad_refl=None), "accumulate=2": dict(accumulate=2), "accumulate=-1": dict(accumulate=-1),
    },
}
# calls that must NOT be refused (without a device the launch fails: any code but GSR_E_INVALID)
ACCEPTED = {
    "gsr_env_scope_forward": {
        "well-formed": {}, "masks-only": dict(MASKS_ONLY), "inside-only": dict(MASKS_ONLY, outside=None), "outside-only": dict(MASKS_ONLY, inside=None),
        "loss-without-inside": dict(inside=None), "radius2=0": dict(radius2=0.0),
    },
    "gsr_env_scope_backward": {"well-formed": {}, "accumulate=1": dict(accumulate=1)},
}
NOOP = {
    "gsr_env_scope_forward": {"P=0-masks-only": dict(MASKS_ONLY, P=0, means3D=None, inside=None, outside=None)},
    "gsr_env_scope_backward": {"P=0": dict(P=0)},
}


def cases():
    out = []
    for entry in ENTRIES[1:]:
        out += [(entry, k, "accepted") for k in ACCEPTED[entry]] + [(entry, k, "noop") for k in NOOP[entry]]
        out += [(entry, k, "refused") for k in REFUSED[entry]]
    return out


def _changes(entry, case):
    for table in (ACCEPTED, NOOP, REFUSED):
        if case in table[entry]:
            return table[entry][case]
    raise KeyError(case)


def _child():
    os.environ.update(cabi_args.HIDE_GPUS)
    sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-reflection_amd"))
    import _gsr
    n = cabi_args._visible_devices()
    print(json.dumps({"devices": n}), flush=True)
    if n != 0:
        return 0
    print(json.dumps({"scratch_floats": int(_gsr.lib.gsr_env_scope_scratch_floats())}), flush=True)
    for entry, case, _ in cases():
        args = dict(BASE[entry], **_changes(entry, case))
        names = FORWARD_ARGS if entry == "gsr_env_scope_forward" else BACKWARD_ARGS
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
        if "scratch_floats" in rec:
            done["scratch_floats"] = rec["scratch_floats"]
        elif "begin" in rec:
            begun = tuple(rec["begin"])
        elif "done" in rec:
            done[tuple(rec["done"])] = rec
            begun = None
    assert p.returncode == 0 and begun is None, f"the child ended in {begun} (exit {p.returncode}):\n{p.stderr[-2000:]}"
    return done


def test_scratch_query_is_positive(outcomes):
    if outcomes is None:
        pytest.skip("a GPU is still visible to the child process although the visible-devices variables hide them: nothing is called")
    assert outcomes["scratch_floats"] > 0 and outcomes["scratch_floats"] % 2 == 0       # whole pairs


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
