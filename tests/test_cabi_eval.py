"""The inference-only surfel forward's C entry (gsr_surfel_forward_eval, ABI 102) on a machine without a GPU: every refusal of it and of
the training forward (gsr_surfel_forward_refl) happens before the first allocation or device call.  Also: the build digest covers every local header the sources include, so that an edit to any of them
rebuilds the library."""
import ctypes
import os
import re

import pytest

import cabi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-splatting-reflection_amd", "csrc")
GSR_E_INVALID = -1


def test_eval_entry_takes_31_arguments(hip_lib_built):
    import _gsr
    args = {name: a for _, name, a in cabi_header.protos("gsr_hip.h")}["gsr_surfel_forward_eval"]
    assert len(args) == 31 == len(_gsr.lib.gsr_surfel_forward_eval.argtypes)


def test_abi_version_is_102(hip_lib_built):
    import _gsr
    hdr = cabi_header.text("gsr_hip.h")
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", hdr).group(1)) == 102
    assert _gsr.GSR_ABI_VERSION == 102
    assert _gsr.lib.gsr_version() == 102


EVAL, TRAIN = "gsr_surfel_forward_eval", "gsr_surfel_forward_refl"


class _Call:
    """A call of one surfel forward entry with well-formed (never dereferenced) pointers; `kw` overrides arguments.  The alloc callback
    records whether the library got as far as asking for workspace."""

    def __init__(self, entry):
        import _gsr
        self.gsr = _gsr
        self.entry = entry
        self.allocs = []
        self.cb = _gsr.ALLOC_FN(lambda user, which, nbytes: self.allocs.append(which) or 0)
        self.fake = 0x7f0000000000        # 256-byte aligned, never touched: every call below must fail validation first

    def __call__(self, **kw):
        f = self.fake
        a = dict(alloc=self.cb, user=None, P=100, D=3, M=16, bg=f, W=64, H=48, means=f, mask=f, shs=f, colors=None, refl_s=f, opac=f, scales=f,
                 mod=1.0, rot=f, tmat=None, view=f, proj=f, campos=f, tx=0.5, ty=0.5, prefiltered=0, color=f, others=f, alpha=f, normal=f,
                 refl_map=f, radii=f, weights=f, refl=None, debug=0, stream=None)
        for k in (("mask", "others", "weights") if self.entry == EVAL else ("alpha", "normal")):
            del a[k]         # (arguments of the other entry)
        assert set(kw) <= set(a), kw
        a.update(kw)
        rc = getattr(self.gsr.lib, self.entry)(*a.values())
        return rc, self.gsr.lib.gsr_last_error().decode()


def _refl_desc(_gsr, **kw):
    f = 0x7f0000000000
    d = dict(cam=f, cubemap=f, fail_value=f, L=16, cubemap_rgba=f, out_final=f, out_refl_color=f, out_normal_world=f, sort_keys=None,
             scratch=None, scratch_floats=0, async_sort=0)
    d.update(kw)
    return ctypes.byref(_gsr.ReflForward(*d.values()))


_CASES = [("alloc", "invalid argument"),
          ("out_color", "invalid argument"),
          ("normal_without_refl", "out_normal_view"),
          ("refl_sort_keys", "sort_keys"),
          ("refl_scratch", "scratch"),
          ("refl_incomplete", "reflection descriptor"),
          ("cubemap_too_large", "cubemap too large"),
          ("means", "missing required input"),
          ("sh_degree", "SH degree"),
          ("shs_misaligned", "16-byte aligned")]
_EVAL_ONLY = ("normal_without_refl", "refl_sort_keys", "refl_scratch")


# (the ids of the eval entry's cases are the ones this test had before it took the training entry)
@pytest.mark.parametrize("entry, case, expect", [pytest.param(EVAL, c, e, id=f"{c}-{e}") for c, e in _CASES] +
                         [pytest.param(TRAIN, c, e, id=f"{TRAIN}-{c}-{e}") for c, e in _CASES if c not in _EVAL_ONLY])
def test_eval_entry_refuses_bad_arguments_before_any_device_call(hip_lib_built, entry, case, expect):
    import _gsr
    call = _Call(entry)
    f = call.fake
    kw = {"alloc": dict(alloc=_gsr.ALLOC_FN()),        # (a NULL function pointer)
          "out_color": dict(color=None),
          "normal_without_refl": dict(normal=None),
          "refl_sort_keys": dict(normal=None, refl=_refl_desc(_gsr, sort_keys=f)),
          "refl_scratch": dict(refl=_refl_desc(_gsr, scratch=f, scratch_floats=1024)),
          "refl_incomplete": dict(refl=_refl_desc(_gsr, out_final=None)),
          "cubemap_too_large": dict(refl=_refl_desc(_gsr, L=30000)),     # 6 L^2 texels do not fit 32 bits
          "means": dict(means=None),
          "sh_degree": dict(D=4),
          "shs_misaligned": dict(shs=f + 4)}[case]
    rc, msg = call(**kw)
    assert rc == GSR_E_INVALID, (case, rc, msg)
    assert expect in msg, (case, msg)
    # the entry that was called: gsr_surfel_forward_eval, or gsr_surfel_forward(_refl) for the training entry
    assert msg.startswith(EVAL + ":" if entry == EVAL else "gsr_surfel_forward"), msg
    assert call.allocs == [], "the entry asked for workspace before refusing"


def _includes_reached(sources):
    seen, todo = set(), list(sources)
    while todo:
        rel = todo.pop()
        text = open(os.path.join(CSRC, rel)).read()
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, flags=re.M):
            r = os.path.normpath(os.path.join(os.path.dirname(rel), inc))
            if r not in seen:
                assert os.path.exists(os.path.join(CSRC, r)), f"{rel} includes missing {inc}"
                seen.add(r)
                todo.append(r)
    return seen


def test_build_digest_covers_every_local_include():
    import sys
    sys.path.insert(0, CSRC)
    import build
    reached = _includes_reached(build.SOURCES)
    assert "gsr_refl.hpp" in reached and os.path.normpath("../../include/gsr_hip.h") in reached
    inputs = {os.path.normpath(p) for p in build.digest_inputs()}
    missing = sorted(reached - inputs)
    assert not missing, f"headers outside the build digest: {missing}"
