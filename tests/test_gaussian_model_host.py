"""scene.GaussianModel and gsr_densification_stats_filter (include/gsr_hip_densify.h) on a machine without a GPU: the class is importable
under both of the reference's names and behaves as the reference's before it has points; the header names the entry's arguments as this
file does, and every refusal the header lists returns GSR_E_INVALID with a message naming the entry.  (That the header, the library and
the binding agree is tests/test_cabi.py's, for every header.)  The calls are made with fake pointers in a child process that sees no GPU
(tests/cabi_child.py); `python test_gaussian_model_host.py` is that child."""
import inspect
import sys

import pytest

import cabi_child
import cabi_header
from cabi_args import FAKE

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
def test_header_names_the_arguments_in_this_order():
    args = {name: a for _, name, a in cabi_header.protos("gsr_hip_densify.h")}[ENTRY]
    assert cabi_header.arg_names(args) == list(ARGS)


def cases():
    return [(k, "refused") for k in REFUSED] + [(k, "noop") for k in NOOPS]


def _call(gsr, entry, case):
    args = dict(BASE, **(REFUSED[case] if case in REFUSED else NOOPS[case]))
    return getattr(gsr.lib, entry)(*[args[k] for k in ARGS])


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    return cabi_child.run(__file__)


@pytest.mark.parametrize("case, expect", cases(), ids=lambda v: v)
def test_refusal(outcomes, case, expect):
    cabi_child.check(outcomes, ENTRY, case, expect)


if __name__ == "__main__":
    sys.exit(cabi_child.serve([(ENTRY, case) for case, _ in cases()], _call))
