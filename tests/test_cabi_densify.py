"""The densification-plan entries (include/gsr_hip_densify.h: gsr_densify_plan_scratch_bytes, gsr_densify_plan_select,
gsr_densify_plan_rows, gsr_prune_rows, gsr_scatter_rows) on a machine without a GPU: the header parses as include/gsr_hip.h does, the
library exports the five, the ctypes prototypes and the plan struct match, the scratch query is what its contract says, and every refusal
the header lists returns GSR_E_INVALID with a message naming the entry.  The calls are made with fake pointers in ONE child process that
hides every GPU and asks the HIP runtime for the device count first (tests/cabi_args.py's guard, by import); with a device still visible
nothing is called.  `python test_cabi_densify.py` is that child."""
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
HEADER = os.path.join(ROOT, "include", "gsr_hip_densify.h")
ENTRIES = ("gsr_densify_plan_scratch_bytes", "gsr_densify_plan_select", "gsr_densify_plan_rows", "gsr_prune_rows", "gsr_scatter_rows")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _protos():
    """[(return type, entry, argument text)] with the regex of tests/test_cabi.py."""
    return re.findall(r"(int|size_t|const char\*)\s+(gsr_\w+)\s*\(([^;]*?)\)\s*;", _source(), flags=re.S)


def test_header_declares_the_entries_and_includes_the_main_header():
    assert sorted(n for _, n, _ in _protos()) == sorted(ENTRIES)
    assert re.search(r'#include "gsr_hip\.h"', open(HEADER).read())
    assert "GSR_ABI_VERSION" not in open(HEADER).read()            # the version is the main header's, and stays


def test_library_exports_them_and_the_lists_are_disjoint(hip_lib_built):
    import _gsr
    raw = ctypes.CDLL(_gsr.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(raw, n), f"{n} declared in gsr_hip_densify.h but not exported by libgsr_hip.so"
    assert sorted(_gsr.EXPORTED_DENSIFY) == sorted(ENTRIES)
    for other in (_gsr.EXPORTED, _gsr.EXPORTED_TRAIN, _gsr.EXPORTED_SCOPE, _gsr.EXPORTED_ENVMAP):
        assert not set(_gsr.EXPORTED_DENSIFY) & set(other)
    for other in ("gsr_hip.h", "gsr_hip_train.h", "gsr_hip_scope.h", "gsr_hip_envmap.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        for n in ENTRIES:
            assert n not in text, (n, other)
    assert _gsr.lib.gsr_version() == _gsr.GSR_ABI_VERSION == 102


def test_ctypes_signatures_and_the_plan_struct_match_the_header(hip_lib_built):
    import _gsr

    def ctype(arg):
        arg = arg.strip()
        if arg.startswith("const gsr_densify_plan*"):
            return ctypes.POINTER(_gsr.DensifyPlan)
        if arg.startswith("const gsr_gather_group*"):
            return ctypes.POINTER(_gsr.GatherGroup)
        if "*" in arg:
            return ctypes.c_void_p
        for pre, t in (("float", ctypes.c_float), ("uint64_t", ctypes.c_uint64), ("size_t", ctypes.c_size_t), ("int", ctypes.c_int)):
            if arg.startswith(pre):
                return t
        raise ValueError(arg)

    for ret, name, args in _protos():
        fn = getattr(_gsr.lib, name)
        assert [ctype(a) for a in args.split(",")] == list(fn.argtypes), name
        assert fn.restype is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int), name
    body = re.search(r"typedef struct \{([^}]*)\}\s*gsr_densify_plan;", _source(), flags=re.S).group(1)
    fields = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        ctype_, name = decl.split()
        base = {"float": ctypes.c_float, "int": ctypes.c_int}[ctype_]
        m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
        fields.append((m.group(1), base * int(m.group(2))) if m else (name, base))
    assert fields == [(n, t) for n, t in _gsr.DensifyPlan._fields_]
    assert ctypes.sizeof(_gsr.DensifyPlan) == 12 * 4


def test_scratch_query(hip_lib_built):
    """Host arithmetic only.  Zero for what the entries refuse; otherwise at least the words and workgroup counts the header's kernel shape
    needs (one word per row and per possible child, twice the rows; 16 bytes per workgroup of 256), growing with P and with N, and without wrap-around at
    the largest P * (N + 1) accepted."""
    import _gsr
    q = _gsr.lib.gsr_densify_plan_scratch_bytes
    for P, N in ((-1, 2), (10, 0), (10, -3), (2 ** 30, 1), (2 ** 31 - 1, 2 ** 31 - 1), (715827883, 2), (1, 2 ** 31 - 1)):
        assert q(P, N) == 0, (P, N)
    assert q(0, 2) > 0
    last = 0
    for P in (1, 255, 256, 257, 65537, 10 ** 6, 2 ** 30 - 1):
        got = q(P, 1)
        assert got >= 4 * (P + 2 * P) + 16 * 3 * ((P + 255) // 256) and got >= last and got % 256 == 0, P
        last = got
    assert q(10 ** 6, 2) >= 4 * (10 ** 6 * 4) and q(10 ** 6, 3) > q(10 ** 6, 2) > q(10 ** 6, 1)
    assert q(715827882, 2) < 4 * 715827882 * (2 + 2) * 1.1         # P * (N + 1) = 2^31 - 2, the largest accepted with N = 2: no wrap-around
    assert q(1, 2 ** 31 - 2) > 0


def test_python_layer_asks_for_a_rebuild_when_the_entries_are_missing(hip_lib_built, monkeypatch):
    import torch

    import gsr_densify
    real = gsr_densify.lib

    class Old:
        """A library built before the densification plan: everything but the five entries."""
        def __getattr__(self, name):
            if name in ENTRIES:
                raise AttributeError(name)
            return getattr(real, name)

    class State:
        """As much of a train state as the checks in front of the library look at."""
        shard = None
        p = {"means3D": torch.zeros(4, 3), "scales": torch.zeros(4, 2), "rotations": torch.zeros(4, 4)}

        class params:
            names = ["means3D", "scales", "rotations"]
            flat = torch.zeros(1)
    monkeypatch.setattr(gsr_densify, "lib", Old())
    with pytest.raises(ImportError, match="rebuild"):
        gsr_densify.densify_and_prune(State, None, 0.0002, 0.05, torch.zeros(3), 3.0, None, plan="device")
    with pytest.raises(ImportError, match="rebuild"):
        gsr_densify.prune_points(State, torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="plan="):
        gsr_densify.densify_and_prune(State, None, 0.0002, 0.05, torch.zeros(3), 3.0, None, plan="host")


# ------------------------------------------------------------------------------------------------- the refusals
P0, N0 = 1000, 2
PLAN0 = dict(max_grad=0.0002, min_weight=0.01, dense_limit=0.03, big_near=0.3, big_far=4.5, extent2=9.0, mean=(0.0, 0.0, 0.0), size_prune=1, N=N0,
             scale_dims=2)
ARGS = {
    "gsr_densify_plan_select": ("P", "plan", "xyz_gradient_accum", "denom", "accum_w", "denom_w", "scaling", "scratch", "scratch_bytes", "counts",
                                "parents", "stream"),
    "gsr_densify_plan_rows": ("P", "plan", "scratch", "scratch_bytes", "xyz", "scaling", "parents", "child_xyz", "child_scaling", "k", "map_param",
                              "map_moment", "child_of", "counts", "stream"),
    "gsr_prune_rows": ("P", "remove", "scratch", "scratch_bytes", "row_map", "counts", "stream"),
    "gsr_scatter_rows": ("src", "dst", "slot", "n_rows", "groups", "num_groups", "stream"),
}
NOT_POINTERS = ("P", "plan", "scratch_bytes", "k", "stream", "n_rows", "groups", "num_groups")
BASE = {e: {a: FAKE for a in ARGS[e] if a not in NOT_POINTERS} for e in ARGS}
BASE["gsr_densify_plan_select"].update(P=P0, plan={}, scratch_bytes="query", stream=None)
BASE["gsr_densify_plan_rows"].update(P=P0, plan={}, scratch_bytes="query", k=10, stream=None)
BASE["gsr_prune_rows"].update(P=P0, scratch_bytes="query1", stream=None)
BASE["gsr_scatter_rows"].update(n_rows=50, groups=((0, 0, 3),), num_groups=1, stream=None)
NAN = float("nan")


def _plan_refusals(pointers):
    out = {
        "P<0": dict(P=-1), "P*(N+1)=2^31": dict(P=2 ** 30, plan=dict(N=1), scratch_bytes=1 << 40),
        "P*(N+1)>2^31:N=3": dict(P=2 ** 29 + 1, plan=dict(N=3), scratch_bytes=1 << 40),
        "P*(N+1)-beyond-32-bits": dict(P=2 ** 31 - 1, plan=dict(N=2 ** 31 - 1), scratch_bytes=1 << 40),
        "null:plan": dict(plan=None), "scale_dims=1": dict(plan=dict(scale_dims=1)), "scale_dims=4": dict(plan=dict(scale_dims=4)),
        "N=0": dict(plan=dict(N=0)), "N<0": dict(plan=dict(N=-2)),
        "max_grad=0": dict(plan=dict(max_grad=0.0)), "max_grad<0": dict(plan=dict(max_grad=-0.0002)), "max_grad=nan": dict(plan=dict(max_grad=NAN)),
        "scratch-one-byte-short": dict(scratch_bytes="query-1"), "scratch=0-bytes": dict(scratch_bytes=0), "misaligned:scratch": dict(scratch=FAKE + 4),
        "P=0:null:counts": dict(P=0, counts=None),
    }
    out.update({f"null:{a}": {a: None} for a in pointers})
    return out


REFUSED = {
    "gsr_densify_plan_select": _plan_refusals(("xyz_gradient_accum", "denom", "accum_w", "denom_w", "scaling", "scratch", "counts", "parents")),
    "gsr_densify_plan_rows": dict(_plan_refusals(("scratch", "xyz", "scaling", "parents", "child_xyz", "child_scaling", "map_param", "map_moment",
                                                  "child_of", "counts")),
                                  **{"k<0": dict(k=-1), "k>P": dict(k=P0 + 1), "P=0:k>0": dict(P=0, k=1)}),
    "gsr_prune_rows": {
        "P<0": dict(P=-1), "P=2^30": dict(P=2 ** 30, scratch_bytes=1 << 40), "null:remove": dict(remove=None), "null:scratch": dict(scratch=None),
        "null:row_map": dict(row_map=None), "null:counts": dict(counts=None), "P=0:null:counts": dict(P=0, counts=None),
        "scratch-one-byte-short": dict(scratch_bytes="query1-1"), "misaligned:scratch": dict(scratch=FAKE + 8),
    },
    "gsr_scatter_rows": {
        "null:src": dict(src=None), "null:dst": dict(dst=None), "null:slot": dict(slot=None), "null:groups": dict(groups=None),
        "num_groups<0": dict(num_groups=-1), "num_groups>16": dict(num_groups=17), "zero-width-group": dict(groups=((0, 0, 0),)),
    },
}
# calls that return 0 without a device: nothing to do
NOOPS = {
    "gsr_scatter_rows": {"n_rows=0": dict(n_rows=0, src=None, dst=None, slot=None), "num_groups=0": dict(num_groups=0, groups=None)},
}


def cases():
    out = []
    for entry in ARGS:
        out += [(entry, k, "refused") for k in REFUSED[entry]] + [(entry, k, "noop") for k in NOOPS.get(entry, {})]
    return out


def _changes(entry, case):
    for table in (REFUSED, NOOPS):
        if case in table.get(entry, {}):
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
    keep = []
    for entry, case, _ in cases():
        args = dict(BASE[entry], **_changes(entry, case))
        if "plan" in args and args["plan"] is not None:
            f = dict(PLAN0, **args["plan"])
            plan = _gsr.DensifyPlan(f["max_grad"], f["min_weight"], f["dense_limit"], f["big_near"], f["big_far"], f["extent2"],
                                    (ctypes.c_float * 3)(*f["mean"]), f["size_prune"], f["N"], f["scale_dims"])
            keep.append(plan)
            args["plan"] = ctypes.byref(plan)
            N = f["N"]
        else:
            N = N0
        sb = args.get("scratch_bytes")
        if isinstance(sb, str):
            query = int(_gsr.lib.gsr_densify_plan_scratch_bytes(args["P"], 1 if sb.startswith("query1") else N))
            query = query or 1 << 40          # (sizes the query itself refuses: the entry must refuse them whatever the scratch)
            args["scratch_bytes"] = query - 1 if sb.endswith("-1") else query
        if args.get("groups") is not None:
            arr = (_gsr.GatherGroup * 17)(*[_gsr.GatherGroup(*(args["groups"][0] if i == 0 else (0, 0, 1))) for i in range(17)])
            keep.append(arr)
            args["groups"] = arr
        print(json.dumps({"begin": [entry, case]}), flush=True)
        rc = getattr(_gsr.lib, entry)(*[args[k] for k in ARGS[entry]])
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
        assert got["rc"] == 0, (entry, case, got)


if __name__ == "__main__":
    sys.exit(_child())
