"""GPU: the two-node deferred reflection pixel by pixel at cube seams and vertices, at every cubemap size that changes its code path, against
the float64 reference chain — with the targeted inputs of tests/helpers_refl.py, every backward path, and no pixel budget: unambiguous pixels
are held to the bars, ambiguous ones (within DELTA of a discontinuity of the lookup) to the envelope of the chain pushed across it.

Cubemap sizes: refl_scratch (csrc/gsr_cubemap.hip) sorts texel ids of key_bits = the smallest b with 2^b > 6 L^2 bits: 8-bit digits up to
L = 104 (16 bits), 9-bit digits (the 512 x 16 shape) for L = 105..209, 10-bit for L = 210..418, three 8-bit passes from L = 419; L = 1024
puts every footprint's lower row beyond the 1024-texel LDS window of refl_run_combine_kernel; L = 1, 2, 3 make (nearly) every footprint a
rim or a vertex."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers_refl as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 16, 104, 105, 128, 209, 210, 418, 419, 1024]


def _summary(inp):
    kinds = np.bincount(inp["kind"], minlength=len(R.KIND_NAMES))
    cls = np.bincount(inp["cls"], minlength=4)
    return dict(L=inp["L"], ambiguous=int(inp["amb"].sum()), ambiguous_random=float(inp["amb"][inp["kind"] == R.K_RANDOM].mean()),
                interior=int(cls[R.INTERIOR]), rim=int(cls[R.RIM]), vertex=int(cls[R.VERTEX]),
                kinds={R.KIND_NAMES[i]: int(n) for i, n in enumerate(kinds) if n})


@pytest.mark.parametrize("L", SIZES)
def test_deferred_reflection_at_seams(L):
    inp = R.seam_inputs(L, seed=L)
    ref = R.reference_run(inp)
    env = R.envelope(inp, ref)
    fails, report = [], dict(_summary(inp), paths={})
    for path in R.PATHS:
        obs, f = R.check_path(inp, ref, env, (R.hip_run(inp, path, False), R.hip_run(inp, path, True)), path)
        report["paths"][path] = {k: round(v, 4) for k, v in obs.items()}
        fails += f
    print("REFL_SEAMS " + json.dumps(report))
    assert not fails, fails


# fast (GSR_REFL_FAST=1, the default: v_rcp / v_rsq / v_sqrt) minus IEEE (GSR_REFL_FAST=0) build on the unambiguous pixels, measured on
# MI355X: `deviation` units (forward planes absolute; gradients relative to their scale).  Bar = 10x the observed value (the suite's convention,
# helpers.N_CONTRIB_BUDGET).
FAST_VS_IEEE_OBSERVED = {
    16: dict(final=1.5e-6, refl=1.7e-6, nworld=1.8e-7, g_nv=5.7e-6, g_base=0.0, g_s=1.9e-6, g_tex=3.4e-6),
    128: dict(final=1.1e-5, refl=1.4e-5, nworld=1.8e-7, g_nv=5.3e-5, g_base=0.0, g_s=1.1e-5, g_tex=2.5e-5),
    1024: dict(final=6.5e-5, refl=1.1e-4, nworld=1.8e-7, g_nv=3.5e-4, g_base=0.0, g_s=8.8e-5, g_tex=2.1e-4),
    "mirror128": dict(final=6.8e-6, refl=9.9e-6, nworld=1.2e-7, g_nv=4.3e-5, g_base=0.0, g_s=3.6e-5, g_tex=1.9e-5)}
FAST_VS_IEEE_SIZES = (16, 128, 1024)


def test_ieee_build_matches_fast_build(tmp_path):
    """The library built with -DGSR_REFL_FAST=0 in every translation unit, run in a fresh process through GSR_LIB: it passes the float64
    checks of test_deferred_reflection_at_seams, and it differs from the default build by no more than the bar."""
    spec = importlib.util.spec_from_file_location("gsr_build", os.path.join(ROOT, "gaussian-splatting-reflection_amd", "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    lib = build.build_variant(str(tmp_path / "ieee"), {"GSR_REFL_FAST": 0})
    out = tmp_path / "dump"
    code = ("import sys; sys.path.insert(0, %r); import helpers_refl as R; R.child_dump(%r, %r)"
            % (os.path.join(ROOT, "tests"), str(out), FAST_VS_IEEE_SIZES))
    env = dict(os.environ, GSR_LIB=lib, GSR_BINDING="ctypes")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    fails, report = [], {}
    for L in FAST_VS_IEEE_SIZES:
        inp = R.seam_inputs(L, seed=L)
        ref = R.reference_run(inp)
        env_ = R.envelope(inp, ref)
        ieee = R.load_dump(str(out / ("L%d.npz" % L)))
        rep = report.setdefault(L, {})
        for p in R.PATHS:
            # (the default build's checks against float64 are test_deferred_reflection_at_seams'; here its outputs feed the deviation)
            fast = (R.hip_run(inp, p, False), R.hip_run(inp, p, True))
            fails += R.check_path(inp, ref, env_, ieee[p], "ieee/" + p)[1]
            for k, v in R.deviation(fast, ieee[p], inp).items():
                rep[k] = max(rep.get(k, 0.0), v)
        for k, v in rep.items():
            bar = 10 * FAST_VS_IEEE_OBSERVED[L][k]
            if v > bar:
                fails.append(("fast vs ieee", L, k, v, bar))
    # the fused node on the mirror scene (L = 128, cone on a cube vertex): the rasterizer's planes are the same in both builds
    inp, fast = R.mirror_case("vertex", 128, False)
    ieee = R.load_dump(str(out / "mirror.npz"), paths=("mirror",))["mirror"]
    assert all(np.array_equal(ieee[0][k], fast[0][k]) for k in ("nv", "base", "strength"))
    ref = R.reference_run(inp)
    fails += R.check_path(inp, ref, R.envelope(inp, ref), ieee, "ieee/mirror")[1]
    rep = report.setdefault("mirror128", R.deviation(fast, ieee, inp))
    for k, v in rep.items():
        if v > 10 * FAST_VS_IEEE_OBSERVED["mirror128"][k]:
            fails.append(("fast vs ieee", "mirror", k, v, FAST_VS_IEEE_OBSERVED["mirror128"][k]))
    print("FAST_VS_IEEE " + json.dumps(report))
    assert not fails, fails


@pytest.mark.parametrize("async_tail", [False, True])
@pytest.mark.parametrize("L", [2, 16, 128])
@pytest.mark.parametrize("target", ["vertex", "edge"])
def test_fused_node_on_mirror_scene(target, L, async_tail):
    """The fused node (rasterize_reflect: the reflection forward as the epilogue of the forward tile kernel, the reflection backward inside
    the node, the texel gradient through a sink) on one nearly opaque surfel in a 2-degree view whose reflected cone is centred on a cube
    vertex or an edge midpoint: the float64 chain on the node's own normal / base / strength planes, the pixel gradients the node hands its
    rasterizer backward, and the sinked texel gradient, with the checks of test_deferred_reflection_at_seams."""
    inp, got = R.mirror_case(target, L, async_tail)
    ref = R.reference_run(inp)
    obs, fails = R.check_path(inp, ref, R.envelope(inp, ref), got, "mirror")
    ok = ~inp["amb"]
    counts = {name: int(((inp["cls"] == c) & ok).sum()) for name, c in (("interior", R.INTERIOR), ("rim", R.RIM), ("vertex", R.VERTEX))}
    print("REFL_MIRROR " + json.dumps(dict(target=target, L=L, async_tail=async_tail, ambiguous=int(inp["amb"].sum()), **counts,
                                           obs={k: round(v, 4) for k, v in obs.items()})))
    if L == 128:      # the cone spans ~4.6 texels: every class present in the hundreds
        assert counts["interior"] >= 100 and counts["rim"] >= 100 and (target != "vertex" or counts["vertex"] >= 100), counts
    assert not fails, fails
