"""The env-scope entries (include/gsr_hip_scope.h: gsr_env_scope_scratch_floats, gsr_env_scope_forward, gsr_env_scope_backward) on a machine
without a GPU: every refusal the header lists returns GSR_E_INVALID with a message naming the entry, and the Python layer asks for a
rebuild when the entries are missing.  (That the header, the library and the binding agree is tests/test_cabi.py's, for every header.)
The calls are made with fake pointers in a child process that sees no GPU (tests/cabi_child.py); `python test_cabi_scope.py` is that
child."""
import sys

import pytest

import cabi_child
from cabi_args import FAKE

ENTRIES = ("gsr_env_scope_scratch_floats", "gsr_env_scope_forward", "gsr_env_scope_backward")


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
TABLES = (("accepted", ACCEPTED), ("noop", NOOP), ("refused", REFUSED))
CASES = cabi_child.cases(ENTRIES[1:], TABLES)         # (the first entry is a size query: it refuses nothing)


def _call(gsr, entry, case):
    args = dict(BASE[entry], **cabi_child.changes(TABLES, entry, case))
    names = FORWARD_ARGS if entry == "gsr_env_scope_forward" else BACKWARD_ARGS
    return getattr(gsr.lib, entry)(*[args[k] for k in names])


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    return cabi_child.run(__file__)


def test_scratch_query_is_positive(hip_lib_built):
    import _gsr
    floats = int(_gsr.lib.gsr_env_scope_scratch_floats())         # (host arithmetic: no device is touched)
    assert floats > 0 and floats % 2 == 0       # whole pairs


@pytest.mark.parametrize("entry, case, expect", CASES, ids=lambda v: v)
def test_refusal(outcomes, entry, case, expect):
    cabi_child.check(outcomes, entry, case, expect)


if __name__ == "__main__":
    sys.exit(cabi_child.serve([c[:2] for c in CASES], _call))
