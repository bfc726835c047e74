"""The densification entries (include/gsr_hip_densify.h: gsr_densify_plan_scratch_bytes, gsr_densify_plan_select, gsr_densify_plan_rows,
gsr_prune_rows, gsr_scatter_rows, and gsr_densification_stats_filter, whose cases tests/test_gaussian_model_host.py holds) on a machine
without a GPU: the header declares these six, the scratch query is what its contract says, the Python layer asks for a rebuild when the
entries are missing, and every refusal the header lists returns GSR_E_INVALID with a message naming the entry.  (That the header, the
library and the binding agree is tests/test_cabi.py's, for every header.)  The calls are made with fake pointers in a child process that
sees no GPU (tests/cabi_child.py); `python test_cabi_densify.py` is that child."""
import ctypes
import sys

import pytest

import cabi_child
import cabi_header
from cabi_args import FAKE

ENTRIES = ("gsr_densify_plan_scratch_bytes", "gsr_densify_plan_select", "gsr_densify_plan_rows", "gsr_prune_rows", "gsr_scatter_rows",
           "gsr_densification_stats_filter")


def test_header_declares_the_six_entries():
    assert sorted(n for _, n, _ in cabi_header.protos("gsr_hip_densify.h")) == sorted(ENTRIES)


def test_the_plan_struct_is_twelve_words(hip_lib_built):
    import _gsr
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
        """A library built before the densification plan: everything but the entries of its header."""
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


_keep = []


def _call(gsr, entry, case):
    args = dict(BASE[entry], **_changes(entry, case))
    if "plan" in args and args["plan"] is not None:
        f = dict(PLAN0, **args["plan"])
        plan = gsr.DensifyPlan(f["max_grad"], f["min_weight"], f["dense_limit"], f["big_near"], f["big_far"], f["extent2"],
                               (ctypes.c_float * 3)(*f["mean"]), f["size_prune"], f["N"], f["scale_dims"])
        _keep.append(plan)
        args["plan"] = ctypes.byref(plan)
        N = f["N"]
    else:
        N = N0
    sb = args.get("scratch_bytes")
    if isinstance(sb, str):
        query = int(gsr.lib.gsr_densify_plan_scratch_bytes(args["P"], 1 if sb.startswith("query1") else N))
        query = query or 1 << 40          # (sizes the query itself refuses: the entry must refuse them whatever the scratch)
        args["scratch_bytes"] = query - 1 if sb.endswith("-1") else query
    if args.get("groups") is not None:
        arr = (gsr.GatherGroup * 17)(*[gsr.GatherGroup(*(args["groups"][0] if i == 0 else (0, 0, 1))) for i in range(17)])
        _keep.append(arr)
        args["groups"] = arr
    return getattr(gsr.lib, entry)(*[args[k] for k in ARGS[entry]])


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    return cabi_child.run(__file__)


@pytest.mark.parametrize("entry, case, expect", cases(), ids=lambda v: v)
def test_refusal(outcomes, entry, case, expect):
    cabi_child.check(outcomes, entry, case, expect)


if __name__ == "__main__":
    sys.exit(cabi_child.serve([c[:2] for c in cases()], _call))
