"""scene.GaussianModel and gsr_densification_stats_filter (include/gsr_hip_densify_stats.h) on a machine without a GPU: the class is
importable under both of the reference's names and behaves as the reference's before it has points; the header declares the entry, the
library exports it, the ctypes prototype matches, and every refusal the header lists returns GSR_E_INVALID with a message naming the
entry.  The calls are made with fake pointers in ONE child process that hides every GPU and asks the HIP runtime for the device count first
(tests/cabi_args.py's guard, as tests/test_cabi_densify.py uses it); with a device still visible nothing is called.
`python test_gaussian_model_host.py` is that child."""
import ctypes
import inspect
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
HEADER = os.path.join(ROOT, "include", "gsr_hip_densify_stats.h")
ENTRY = "gsr_densification_stats_filter"
ARGS = ("P", "grad_means2D", "update_filter", "gaussian_weights", "xyz_gradient_accum", "denom", "accum_w", "denom_w", "stream")
POINTERS = ARGS[1:-1]
P0 = 1031
BASE = dict({a: FAKE for a in POINTERS}, P=P0, stream=None)
REFUSED = dict({"P<0": dict(P=-1), "P<0:null-buffers": dict({a: None for a in POINTERS}, P=-7)}, **{f"null:{a}": {a: None} for a in POINTERS})
NOOPS = {"P=0": dict(P=0), "P=0:null-buffers": dict({a: None for a in POINTERS}, P=0)}


# ------------------------------------------------------------------------------------------------- the class
def test_the_class_is_importable_under_both_of_the_reference_names(hip_lib_built):
    from scene import GaussianModel as from_scene
    from gaussian_renderer import GaussianModel as from_renderer
    from scene.gaussian_model import GaussianModel
    assert from_scene is from_renderer is GaussianModel


def test_constructor_and_keyword_only_extensions(hip_lib_built):
    """The constructor is the reference's; whatever the reference's methods do not have is keyword-only."""
    from scene import GaussianModel
    sig = inspect.signature(GaussianModel.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("sh_degree", inspect.Parameter.empty), ("init_refl_value", 1e-3),
                                                                                 ("init_cubemap_resol", 128)]
    reference = {"create_from_pcd": ["pcd", "spatial_lr_scale", "init_refl_value", "init_opacity_value"], "training_setup": ["training_args"],
                 "add_densification_stats": ["viewspace_point_tensor", "update_filter", "render_weight"],
                 "densify_and_prune": ["max_grad", "min_opacity", "mean", "extent", "max_screen_size"], "prune_points": ["mask"],
                 "prune_points_no_grad": ["mask"], "reset_opacity": ["reset_value", "exclusive_msk"], "reset_refl": ["exclusive_msk"],
                 "reset_scale": ["enlarge_scale", "exclusive_msk"], "dist_color": ["noise_range", "exclusive_msk"], "get_covariance": ["scaling_modifier"],
                 "restore": ["model_args", "training_args"], "save_ply": ["path"], "load_ply": ["path"], "set_opacity_lr": ["lr"],
                 "update_learning_rate": ["iteration"], "double_env_map": [], "filter_env_map": [], "freeze_xyz": [], "oneupSHdegree": [], "capture": []}
    for name, positional in reference.items():
        params = list(inspect.signature(getattr(GaussianModel, name)).parameters.values())[1:]
        assert [p.name for p in params if p.kind is p.POSITIONAL_OR_KEYWORD] == positional, name
        assert all(p.kind is p.KEYWORD_ONLY for p in params if p.name not in positional), name
    assert list(inspect.signature(GaussianModel.bind).parameters)[1] == "pipe"


def test_a_model_without_points_is_the_reference_s_empty_model(hip_lib_built):
    from scene import GaussianModel
    m = GaussianModel(3, init_cubemap_resol=8)
    assert m.optimizer is None and m.active_sh_degree == 0 and m.max_sh_degree == 3 and m.env_map_resol == 8 and m.env_map is None
    assert m.percent_dense == 0 and m.spatial_lr_scale == 0 and m.init_refl_value == 1e-3
    for name in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_refl_strength", "max_radii2D",
                 "xyz_gradient_accum", "denom", "accum_w", "denom_w", "get_xyz", "get_opacity"):
        assert getattr(m, name).numel() == 0, name
    for _ in range(5):
        m.oneupSHdegree()
    assert m.active_sh_degree == 3
    with pytest.raises(RuntimeError, match="training_setup"):
        m.densify_and_prune(0.0002, 0.05, (0.0, 0.0, 0.0), 3.0, None)
    with pytest.raises(RuntimeError, match="no points"):
        m.training_setup(None)


# ------------------------------------------------------------------------------------------------- the entry
def _protos():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.findall(r"(int|size_t|const char\*)\s+(gsr_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)


def test_header_library_and_prototype_agree(hip_lib_built):
    import _gsr
    protos = _protos()
    assert [n for _, n, _ in protos] == [ENTRY]
    ret, _, args = protos[0]
    assert [re.sub(r".*[\s\*]", "", a.strip()) for a in args.split(",")] == list(ARGS)
    assert "GSR_ABI_VERSION" not in open(HEADER).read() and _gsr.lib.gsr_version() == _gsr.GSR_ABI_VERSION == 102
    assert hasattr(ctypes.CDLL(_gsr.LIB_PATH), ENTRY), f"{ENTRY} is not exported by libgsr_hip.so"
    fn = getattr(_gsr.lib, ENTRY)
    assert list(fn.argtypes) == [ctypes.c_void_p if "*" in a else ctypes.c_int for a in args.split(",")] and fn.restype is ctypes.c_int and ret == "int"
    assert _gsr.EXPORTED_DENSIFY_STATS == [ENTRY]
    for other in (_gsr.EXPORTED, _gsr.EXPORTED_TRAIN, _gsr.EXPORTED_SCOPE, _gsr.EXPORTED_ENVMAP, _gsr.EXPORTED_DENSIFY):
        assert ENTRY not in other
    # a host that includes the densification header has the whole interface
    assert re.search(r'#include "gsr_hip_densify_stats\.h"', open(os.path.join(ROOT, "include", "gsr_hip_densify.h")).read())


def cases():
    return [(k, "refused") for k in REFUSED] + [(k, "noop") for k in NOOPS]


def _child():
    os.environ.update(cabi_args.HIDE_GPUS)
    sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-reflection_amd"))
    import _gsr
    n = cabi_args._visible_devices()
    print(json.dumps({"devices": n}), flush=True)
    if n != 0:
        return 0
    for case, _ in cases():
        args = dict(BASE, **(REFUSED[case] if case in REFUSED else NOOPS[case]))
        print(json.dumps({"begin": case}), flush=True)
        rc = getattr(_gsr.lib, ENTRY)(*[args[k] for k in ARGS])
        msg = _gsr.lib.gsr_last_error()
        print(json.dumps({"done": case, "rc": int(rc), "msg": msg.decode(errors="replace") if msg else ""}), flush=True)
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
            begun = rec["begin"]
        elif "done" in rec:
            done[rec["done"]] = rec
            begun = None
    assert p.returncode == 0 and begun is None, f"the child ended in {begun} (exit {p.returncode}):\n{p.stderr[-2000:]}"
    return done


@pytest.mark.parametrize("case, expect", cases(), ids=lambda v: v)
def test_refusal(outcomes, case, expect):
    if outcomes is None:
        pytest.skip("a GPU is still visible to the child process although the visible-devices variables hide them: nothing is called")
    got = outcomes.get(case)
    assert got is not None, "the child never reached this call"
    if expect == "refused":
        assert got["rc"] == GSR_E_INVALID, (case, got)
        assert got["msg"].startswith(ENTRY), (case, got["msg"])
    else:
        assert got["rc"] == 0, (case, got)


if __name__ == "__main__":
    sys.exit(_child())
