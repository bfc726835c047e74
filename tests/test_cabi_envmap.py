"""The environment-map entries (include/gsr_hip_envmap.h: gsr_envmap_resize, gsr_envmap_sharpen) on a machine without a GPU: the header
parses as include/gsr_hip.h does, the library exports the two, the ctypes prototypes match, and every refusal the header lists returns
GSR_E_INVALID with a message naming the entry.  The calls are made with fake pointers in ONE child process that hides every GPU and asks
the HIP runtime for the device count first (tests/cabi_args.py's guard, by import); with a device still visible nothing is called.
`python test_cabi_envmap.py` is that child."""
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
HEADER = os.path.join(ROOT, "include", "gsr_hip_envmap.h")
ENTRIES = ("gsr_envmap_resize", "gsr_envmap_sharpen")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _protos():
    """[(return type, entry, argument text)] with the regex of tests/test_cabi.py."""
    return re.findall(r"(int|size_t|const char\*)\s+(gsr_\w+)\s*\(([^;]*?)\)\s*;", _source(), flags=re.S)


def test_header_declares_the_two_entries_and_includes_the_main_header():
    assert sorted(n for _, n, _ in _protos()) == sorted(ENTRIES)
    assert re.search(r'#include "gsr_hip\.h"', open(HEADER).read())
    assert "GSR_ABI_VERSION" not in open(HEADER).read()            # the version is the main header's, and stays


def test_library_exports_them_and_the_lists_are_disjoint(hip_lib_built):
    import _gsr
    raw = ctypes.CDLL(_gsr.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(raw, n), f"{n} declared in gsr_hip_envmap.h but not exported by libgsr_hip.so"
    assert sorted(_gsr.EXPORTED_ENVMAP) == sorted(ENTRIES)
    for other in (_gsr.EXPORTED, _gsr.EXPORTED_TRAIN, _gsr.EXPORTED_SCOPE):
        assert not set(_gsr.EXPORTED_ENVMAP) & set(other)
    for other in ("gsr_hip.h", "gsr_hip_train.h", "gsr_hip_scope.h"):
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
        assert [ctype(a) for a in args.split(",")] == list(fn.argtypes), name
        assert fn.restype is ctypes.c_int, name


def test_python_layer_asks_for_a_rebuild_when_the_entries_are_missing(hip_lib_built, monkeypatch):
    import gsr_envmap
    real = gsr_envmap.lib

    class Old:
        """A library built before the environment-map transforms: everything but the two entries."""
        def __getattr__(self, name):
            if name in ENTRIES:
                raise AttributeError(name)
            return getattr(real, name)

    class State:
        """As much of a train state as the checks in front of the library look at."""
        shard = None

        class params:
            names = ["means3D", "cubemap", "fail"]
            shapes = {"cubemap": (6, 3, 4, 4)}
    monkeypatch.setattr(gsr_envmap, "lib", Old())
    for call in (lambda: gsr_envmap.resize_env_map(State, 8), lambda: gsr_envmap.double_env_map(State), lambda: gsr_envmap.filter_env_map(State)):
        with pytest.raises(ImportError, match="rebuild"):
            call()


# ------------------------------------------------------------------------------------------------- the refusals
RESIZE_ARGS = ("src", "dst", "planes", "L_src", "L_dst", "stream")
SHARPEN_ARGS = ("src", "dst", "planes", "L", "factor", "lo", "hi", "stream")
FAR = FAKE + (1 << 36)              # a second fake range that the largest source of these cases (8 GiB) does not reach
BASE = {
    "gsr_envmap_resize": dict(src=FAKE, dst=FAR, planes=18, L_src=128, L_dst=256, stream=None),
    "gsr_envmap_sharpen": dict(src=FAKE, dst=FAR, planes=18, L=128, factor=2.0, lo=1e-3, hi=1 - 1e-3, stream=None),
}
INF, NAN = float("inf"), float("nan")
SRC_BYTES = 18 * 128 * 128 * 4       # of both base calls
REFUSED = {
    "gsr_envmap_resize": {
        "null:src": dict(src=None), "null:dst": dict(dst=None), "misaligned:src": dict(src=FAKE + 2), "misaligned:dst": dict(dst=FAR + 1),
        "planes=0": dict(planes=0), "planes<0": dict(planes=-6), "L_src=0": dict(L_src=0), "L_src<0": dict(L_src=-1), "L_dst=0": dict(L_dst=0),
        "L_dst<0": dict(L_dst=-256),
        "src:planes*L*L=2^31": dict(planes=2, L_src=32768, L_dst=4), "dst:planes*L*L=2^31": dict(planes=2, L_src=4, L_dst=32768),
        "dst:planes*L*L-beyond-64-bits": dict(planes=2 ** 31 - 1, L_src=1, L_dst=2 ** 31 - 1),
        "overlap:same": dict(dst=FAKE), "overlap:dst-starts-in-the-last-src-texel": dict(dst=FAKE + SRC_BYTES - 4),
        "overlap:src-starts-in-the-last-dst-texel": dict(src=FAR + 4 * SRC_BYTES - 4),
    },
    "gsr_envmap_sharpen": {
        "null:src": dict(src=None), "null:dst": dict(dst=None), "misaligned:src": dict(src=FAKE + 1), "misaligned:dst": dict(dst=FAR + 2),
        "planes=0": dict(planes=0), "planes<0": dict(planes=-1), "L=0": dict(L=0), "L<0": dict(L=-128),
        "planes*L*L=2^31": dict(planes=2, L=32768), "planes*L*L-beyond-64-bits": dict(planes=2 ** 31 - 1, L=2 ** 31 - 1),
        "overlap:same": dict(dst=FAKE), "overlap:dst-starts-in-the-last-src-texel": dict(dst=FAKE + SRC_BYTES - 4),
        "overlap:src-starts-in-the-last-dst-texel": dict(src=FAR + SRC_BYTES - 4),
        "factor=inf": dict(factor=INF), "factor=-inf": dict(factor=-INF), "factor=nan": dict(factor=NAN),
        "lo=0": dict(lo=0.0), "lo<0": dict(lo=-1e-3), "lo=hi": dict(lo=0.5, hi=0.5), "lo>hi": dict(lo=0.75, hi=0.25), "hi=1": dict(hi=1.0),
        "hi>1": dict(hi=1.5), "lo=nan": dict(lo=NAN), "hi=nan": dict(hi=NAN),
    },
}
# calls that must NOT be refused (without a device the launch fails: any code but GSR_E_INVALID)
ACCEPTED = {
    "gsr_envmap_resize": {
        "well-formed": {}, "shrink": dict(L_src=7, L_dst=3), "same-size": dict(L_dst=128), "to-one-texel": dict(L_dst=1), "from-one-texel": dict(L_src=1),
        "one-plane": dict(planes=1), "largest": dict(planes=2, L_src=4, L_dst=32767), "dst-right-behind-src": dict(dst=FAKE + SRC_BYTES),
        "src-right-behind-dst": dict(src=FAR + 4 * SRC_BYTES),
    },
    "gsr_envmap_sharpen": {
        "well-formed": {}, "L=1": dict(L=1), "L=2": dict(L=2), "factor=0": dict(factor=0.0), "factor<0": dict(factor=-1.0),
        "largest": dict(planes=2, L=32767), "dst-right-behind-src": dict(dst=FAKE + SRC_BYTES), "wide-clamp": dict(lo=1e-6, hi=1 - 1e-6),
    },
}


def cases():
    out = []
    for entry in ENTRIES:
        out += [(entry, k, "accepted") for k in ACCEPTED[entry]] + [(entry, k, "refused") for k in REFUSED[entry]]
    return out


def _changes(entry, case):
    for table in (ACCEPTED, REFUSED):
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
    for entry, case, _ in cases():
        args = dict(BASE[entry], **_changes(entry, case))
        names = RESIZE_ARGS if entry == "gsr_envmap_resize" else SHARPEN_ARGS
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
    else:
        assert got["rc"] != GSR_E_INVALID, (entry, case, got)


if __name__ == "__main__":
    sys.exit(_child())
