"""GPU: paths that the default build reaches only at sizes no test affords, run at small sizes by a build that moves their thresholds:
  S_CAP = 32                 the surfel backward cuts a batch with more than S_CAP (4x4 sub-block, entry) pairs at multiples of 8
                             positions.  On the surface family's test scene (3000 surfels, 200x136) 37 % of the (8x8 block, 64-entry
                             batch) units carry more than 32 pairs and 21 % more than 48, the default (adversarial_scenes.reach, the
                             count of tests/blend_stats.py), so the cut runs in both builds; at 32 it runs more often and deeper.
  TILE_SORT_SMALL_FROM = 1   every tile sort takes the SMALL shapes (1024 x 8 items per block) that the default build keeps for
                             9 M instances and more: 8-bit digits (TILE_SORT_SHAPE_SMALL) below 8 and above 14 tile-id bits, 7-bit
                             digits (TILE_SORT_SHAPE_SMALL7) between.  The grids straddle both edges: 127 tiles (7 bits, one 7-bit pass)
                             against 128 (8 bits: a 7-bit and a 1-bit pass), 16 383 tiles (14 bits: two full 7-bit passes) against
                             16 384 (15 bits: an 8-bit and a 7-bit pass); instance counts 8191 / 8192 / 8193 sit on the SMALL block.
The library is built once per session with those defines (csrc/build.py build_variant) and loaded in a fresh child process through
GSR_LIB; the child runs the oracle checks of tests/test_gpu_adversarial.py and reports which library it loaded."""
import importlib.util
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFINES = {"S_CAP": 32, "TILE_SORT_SMALL_FROM": 1}


@pytest.fixture(scope="module")
def rare_lib(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("gsr_build", os.path.join(ROOT, "gaussian-splatting-reflection_amd", "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build.build_variant(str(tmp_path_factory.mktemp("rare_paths")), DEFINES)


def child(case):
    """Runs in the child process (GSR_LIB = the variant build)."""
    import _gsr
    import adversarial_scenes as A
    import test_gpu_adversarial as T
    lib = os.environ["GSR_LIB"]
    assert os.path.samefile(_gsr.LIB_PATH, lib), (_gsr.LIB_PATH, lib)
    print("RARE_PATHS child uses %s (%s)" % (_gsr.LIB_PATH, " ".join("%s=%s" % kv for kv in sorted(DEFINES.items()))), flush=True)
    if case in ("surface", "threshold", "dup_surface"):
        P, W, H, seed = A.SCENES[case]
        T.check_surfel(A.family(case, "S", P, W, H, seed), seed)
    elif case.startswith("grid"):
        W, H, P = {"grid127": (2032, 16, 3000), "grid128": (2048, 16, 3000), "grid16383": (2064, 2032, 20000),
                   "grid16384": (2048, 2048, 20000)}[case]
        for variant in ("S", "G"):
            T.check_exact_binning(variant, T.exact_instances(variant, P, W, H, P + W), P)
        T.check_exact_binning("S", T.exact_instances("S", P, W, H, P + W + 1, dup=True), P)
    else:
        P = int(case[1:])
        T.check_exact_binning("S", T.exact_instances("S", P, 328, 232, P), P)
    print("RARE_PATHS %s ok" % case, flush=True)


@pytest.mark.parametrize("case", ["surface", "threshold", "dup_surface", "grid127", "grid128", "grid16383", "grid16384", "n8191", "n8192",
                                  "n8193"])
def test_rare_path_build_against_oracle(rare_lib, case):
    code = "import sys; sys.path[:0] = %r; import test_gpu_rare_paths as R; R.child(%r)" % (
        [ROOT, os.path.join(ROOT, "gaussian-splatting-reflection_amd"), os.path.join(ROOT, "tests")], case)
    env = dict(os.environ, GSR_LIB=rare_lib, GSR_BINDING="ctypes")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "RARE_PATHS child uses" in r.stdout and ("RARE_PATHS %s ok" % case) in r.stdout
