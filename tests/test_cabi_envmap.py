"""The environment-map entries (include/gsr_hip_envmap.h: gsr_envmap_resize, gsr_envmap_sharpen) on a machine without a GPU: every refusal
the header lists returns GSR_E_INVALID with a message naming the entry, and the Python layer asks for a rebuild when the entries are
missing.  (That the header, the library and the binding agree is tests/test_cabi.py's, for every header.)  The calls are made with fake
pointers in a child process that sees no GPU (tests/cabi_child.py); `python test_cabi_envmap.py` is that child."""
import sys

import pytest

import cabi_child
from cabi_args import FAKE

ENTRIES = ("gsr_envmap_resize", "gsr_envmap_sharpen")


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
TABLES = (("accepted", ACCEPTED), ("refused", REFUSED))
CASES = cabi_child.cases(ENTRIES, TABLES)


def _call(gsr, entry, case):
    args = dict(BASE[entry], **cabi_child.changes(TABLES, entry, case))
    names = RESIZE_ARGS if entry == "gsr_envmap_resize" else SHARPEN_ARGS
    return getattr(gsr.lib, entry)(*[args[k] for k in names])


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    return cabi_child.run(__file__)


@pytest.mark.parametrize("entry, case, expect", CASES, ids=lambda v: v)
def test_refusal(outcomes, entry, case, expect):
    cabi_child.check(outcomes, entry, case, expect)


if __name__ == "__main__":
    sys.exit(cabi_child.serve([c[:2] for c in CASES], _call))
