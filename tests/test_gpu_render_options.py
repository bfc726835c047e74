"""render() and render_fast() of gaussian_renderer under every option of their signatures, and GaussianRasterizer.markVisible, against
tests/render_ref.py (the reference's render() restated from the oracle and the float64 chains; pinned by tests/test_render_ref.py).

The rest of the suite drives render() at scaling_modifier 1.0, without override_color, without an env-scope radius and with
pipe.compute_cov3D_python False.  Here, on ONE small scene (3000 surfels, 200x136 = ragged tiles, cubemap 16, an off-axis rolled camera with
FoVx != FoVy), one forward and one backward per case, each with FUSED_REFLECTION on and off:

  default, initial, scope (+ initial), colour, mod-small / mod-large, pycov / pycov-mod, depth-ratio 0.3 / 1.0, sh-low

compared in the staged way of tests/test_gpu_fullsize_fused.py, so that a float32-against-float64 texel-cell flip does not compound:

  A  the rasterizer's outputs against the float32 oracle given the same arguments (tests/test_gpu_parity.py's bars for variant S);
  B  the pixel passes against the float64 chains evaluated on the HIP rasterizer's OWN planes;
  C  the gradients of render_ref.loss: the pixel gradients the HIP pixel passes hand the rasterizer backward against float64 autograd of the
     chains, then every parameter gradient against the oracle's backward fed with those captured pixel gradients;
  D  (pycov) the gradients that reach position, scale and raw quaternion through _precomputed_transmats and pc.get_covariance against
     float64 autograd of transmats_ref o get_covariance_ref fed with the oracle's dL_dtransMat, plus the oracle's direct dL_dmeans3D.

E: at a scaling modifier other than 1 the reference's surfel backward rebuilds T with modifier 1 (DSR backward.cu:511); the oracle
reproduces that (tests/test_gpu_api_paths.py::test_scale_modifier), so stage C holds the HIP backward to the same quirk.  It is the
reference's behaviour, not a bug to fix here.

Every tolerance is that of a named existing test of the same quantity:
  colour 3e-5 with helpers.assert_image_close, planes >= 50 dB, gaussian_weights       tests/test_gpu_parity.py::_run_surfel
  surf_depth rtol 1e-5 / atol 1e-6, surf_normal 5e-4, rend_normal 1e-5 (initial stage)  test_gpu_surface.py::test_render_surface_outputs_equal_torch_chain
  render, refl_color_map, rend_normal 2e-5                                             test_gpu_fullsize_fused.py::test_c3_fused_step_against_chain_and_oracle
  pixel gradients: normal 1e-3 of max on all but 2e-3 of the pixels, base 1e-5, strength 1e-4      test_gpu_fullsize_fused.py::_oracle_view
  allmap gradient of the surface pass 1e-3 of the plane's max                          test_gpu_surface.py::test_surface_pass_matches_golden
  parameter gradients rel_maxnorm 1e-4 and grad_gate <= GATE_BUDGET, cubemap 1e-4, fail value 1e-7 + 1e-5 max     the c3 test above
The one bound that has no such test, that of the Python homographies themselves, is 4 x what the reference alone measures (_check_transmats).
Each figure is printed before it is asserted (pytest -s shows them).
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import render_ref as RR
from helpers import GATE_BUDGET, S, assert_image_close, assert_planes_psnr, grad_gate, n_contrib_ok, psnr, rel_maxnorm
from test_gpu_dropin import _Pipe, _model, _view

pytestmark = pytest.mark.gpu

P, W, H, L, SEED, MU = 3000, 200, 136, 16, 5, -2.8
BG = (0.1, 0.2, 0.3)
SCOPE = dict(env_scope_center=(0.5, 0.2, 5.0), env_scope_radius=1.6)
NAMES = ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")
ORACLE_NAMES = dict(means3D="dL_dmeans3D", shs="dL_dsh", opacities="dL_dopacity", scales="dL_dscales", rotations="dL_drotations",
                    refl_strengths="dL_drefl_strengths")

CASES = {
    "default": {},
    "initial": dict(initial_stage=True),
    "scope": dict(SCOPE),
    "scope-initial": dict(SCOPE, initial_stage=True),
    "colour": dict(colour=True),
    "mod-small": dict(scaling_modifier=0.7),
    "mod-large": dict(scaling_modifier=1.6),
    "pycov": dict(compute_cov3D_python=True),
    "pycov-mod": dict(compute_cov3D_python=True, scaling_modifier=1.3),
    "depth-ratio-0.3": dict(depth_ratio=0.3),
    "depth-ratio-1.0": dict(depth_ratio=1.0),
    "sh-low": dict(sh_degree=1),
}


def _camera():
    return S.look_at_camera(W, H, eye=(0.4, -0.3, -1.0), target=(0, 0, 5))


@functools.lru_cache(maxsize=None)
def _data():
    """The scene as numpy (never modified): make_scene's surfels with RAW quaternions (lengths 0.5 to 2: the rasterizer normalises inside,
    get_covariance through build_rotation), the cubemap, seeded override colours."""
    rs = np.random.RandomState(SEED)
    sc = {k: v for k, v in S.make_scene(P, "S", seed=SEED, mu=MU).items() if k in NAMES}
    sc["rotations"] = (sc["rotations"] * rs.uniform(0.5, 2.0, (P, 1))).astype(np.float32)
    tex, fail = S.make_cubemap(L, 3, SEED)
    return sc, tex, fail + np.float32(0.25), rs.rand(P, 3).astype(np.float32)


class _Env:
    def __init__(self, tex, fail):
        self.params = {"Cubemap_texture": tex, "Cubemap_failv": fail}


def _setup(sh_degree=3, compute_cov3D_python=False, depth_ratio=0.0, requires_grad=True):
    sc, tex, fail, colours = _data()
    cam = _camera()
    leaf = lambda a: torch.from_numpy(a).cuda().requires_grad_(requires_grad)
    t = {k: leaf(sc[k]) for k in NAMES}
    t["cubemap"], t["fail"], t["colours"] = leaf(tex), leaf(fail), leaf(colours)

    class PC(_model(t, _Env(t["cubemap"], t["fail"]), sh_degree)):
        @staticmethod
        def get_covariance(scaling_modifier=1):
            return RR.get_covariance_ref(t["means3D"], t["scales"], t["rotations"], scaling_modifier)

    class Pipe(_Pipe):
        pass
    Pipe.depth_ratio, Pipe.compute_cov3D_python = depth_ratio, compute_cov3D_python
    return cam, _view(cam, W, H), PC, Pipe, t, torch.tensor(BG, device="cuda")


def _npy(t):
    return t.detach().cpu().numpy()


def _fig(what, value, bound):
    print("FIG %-40s %.3e (bound %.3e)" % (what, value, bound))
    return value <= bound


def _stage_a(pkg, fo, initial_stage):
    """Rasterizer outputs of render() against the float32 oracle's (tests/test_gpu_parity.py::_run_surfel)."""
    base = pkg["render"] if initial_stage else pkg["base_color_map"]
    allmap = _npy(pkg["rend_alpha"]._base)
    assert allmap.shape == (8, H, W)
    assert base.grad_fn.num_rendered == fo["num_rendered"]
    np.testing.assert_array_equal(_npy(pkg["radii"]), fo["radii"])
    assert torch.equal(pkg["visibility_filter"], pkg["radii"] > 0)
    assert _fig("A base colour psnr deficit", 50.0 - psnr(_npy(base), fo["color"]), 0.0)
    print("FIG A base colour max-abs %.3e" % np.abs(_npy(base) - fo["color"]).max())
    assert_image_close(_npy(base), fo["color"], 3e-5)
    assert_planes_psnr(allmap, fo["allmap"])
    for k, plane in (("rend_alpha", 1), ("rend_dist", 6), ("env_scope_mask", 7)):
        assert torch.equal(pkg[k], pkg["rend_alpha"]._base[plane:plane + 1]), k
    if not initial_stage:
        assert psnr(_npy(pkg["refl_strength_map"]), fo["refl_strength_map"]) >= 50.0
    mask = allmap[7]
    assert set(np.unique(mask)) <= {0.0, 1.0}
    assert n_contrib_ok(mask, fo["allmap"][7])
    gw_h, gw_o = _npy(pkg["gaussian_weights"]).astype(np.float64), fo["gaussian_weights"].astype(np.float64)
    gw_bad = np.abs(gw_h - gw_o) > 1.5e-6 + 1e-5 * np.abs(gw_o)
    assert int(gw_bad.sum()) <= max(2, int(3e-5 * gw_o.size)) and np.abs(gw_h - gw_o).max() <= 5e-3
    return allmap


def _stage_b(pkg, maps, initial_stage):
    """The pixel passes against the float64 chains on the HIP rasterizer's own planes."""
    assert set(pkg.keys()) == (RR.KEYS_INITIAL if initial_stage else RR.KEYS_FULL)
    sd, sd_r = _npy(pkg["surf_depth"]), _npy(maps["surf_depth"])
    ok = _fig("B surf_depth / (1e-6 + 1e-5 |ref|)", float((np.abs(sd - sd_r) / (1e-6 + 1e-5 * np.abs(sd_r))).max()), 1.0)
    ok &= _fig("B surf_normal", float(np.abs(_npy(pkg["surf_normal"]) - _npy(maps["surf_normal"])).max()), 5e-4)
    ok &= _fig("B rend_normal", float(np.abs(_npy(pkg["rend_normal"]) - _npy(maps["rend_normal"])).max()), 1e-5 if initial_stage else 2e-5)
    for k in () if initial_stage else ("render", "refl_color_map"):
        ok &= _fig("B " + k, float(np.abs(_npy(pkg[k]) - _npy(maps[k])).max()), 2e-5)
    assert ok


@contextlib.contextmanager
def _captured(pkg, fused, initial_stage):
    """The pixel gradients the HIP pixel passes hand the rasterizer backward: {g_base, g_strength, g_normal_view, allmap}.  Fused node: its
    test probe; two nodes: tensor hooks on the rasterizer's outputs, and, for the normal planes (an output tap of the rasterizer, which
    render() does not return), the gradient the pixel pass's node returns for its first input."""
    import gaussian_renderer as GR
    cap = {}
    keep = lambda name: (lambda g: cap.__setitem__(name, g.detach().clone()))
    pkg["rend_alpha"]._base.register_hook(keep("allmap"))
    if fused:
        GR._RasterizeReflect.probe = cap
    else:
        (pkg["render"] if initial_stage else pkg["base_color_map"]).register_hook(keep("g_base"))
        if not initial_stage:
            pkg["refl_strength_map"].register_hook(keep("g_strength"))
        pkg["rend_normal"].grad_fn.register_hook(lambda grad_inputs, grad_outputs: cap.__setitem__("g_normal_view", grad_inputs[0].detach().clone()))
    try:
        yield cap
    finally:
        GR._RasterizeReflect.probe = None


def _gate(what, got, want, floor=1e-6):
    got, want = np.asarray(got), np.asarray(want)
    ok = _fig("C %s rel_maxnorm" % what, rel_maxnorm(got.reshape(want.shape), want), 1e-4)
    return _fig("C %s grad_gate" % what, grad_gate(got, want, floor=floor), GATE_BUDGET) and ok


def _needed_floor(got, want):
    """The smallest `floor` with which helpers.grad_gate(got, want) leaves no element out."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(((np.abs(got.reshape(want.shape) - want) - 1e-4 * np.abs(want)) / np.abs(want).max()).max())


# The two gradients of the pycov cases that miss the floor of helpers.grad_gate (1e-6 of the tensor's maximum), each by ONE element, while
# every other tensor of every case meets it (the scale gradient at modifier 1.3 needs 0.995e-6 on one run and the sum order changes from run
# to run, so it is counted with the one at 1.0).  Both are entries of the rasterizer's dL_dtransMat seen through a large factor: the scale
# gradient contracts it with world2pix, whose entries are the size of the focal length in pixels (six such products that largely cancel);
# the screen-space gradient is one entry of it times depth * W / 2 (DSR backward.cu:656-659).  dL_dtransMat is a sum over pixels that the GPU
# forms in another order than the oracle; its rounding reaches a small element at a few 1e-6 of the maximum.  The reference alone, measured on
# the CPU in the same way (float32 oracle against float64 oracle on the same inputs, homographies and upstream gradients, the scale gradient
# pulled back through render_ref.python_path_gradients on both sides), needs a floor of 4.93e-6 / 1.87e-6 for the scale gradient at modifier 1.0 / 1.3
# and of 1.81e-4 for the screen-space gradient at modifier 1.3 (the GPU needed 2.8e-6 / 1.0e-6 and 1.3e-6).  The floor of these two is 4 x that measurement; rtol, GATE_BUDGET and the 1e-4
# of rel_maxnorm stay, and so does 1e-6 for every other tensor (the reference alone would need 1.1e-4 for the position and 5.5e-5 for the
# quaternion gradient, which the HIP path does not).  What the GPU needed: see "smallest floor that passes" in the output.
PYTHON_PATH_FLOOR = {("scales", 1.0): 4 * 4.93e-6, ("scales", 1.3): 4 * 1.87e-6, ("viewspace_points", 1.3): 4 * 1.81e-4}


def _check_transmats(T, sc, cam, modifier):
    """The homographies render() handed the rasterizer (float32, formed on the device by _precomputed_transmats from pc.get_covariance)
    against transmats_ref o get_covariance_ref in float64.  T[p] = (three rows of the splat matrix) @ (three columns of world2pix): an entry
    is a 4-term dot product whose terms are bounded by (largest entry of the row) * |world2pix column|, so its float32 error is measured
    in units of u * rowmax_i * sum_k |world2pix[k, j]| with u = 2^-24.  The reference alone (the same torch code in float32 against
    float64, on the CPU) reaches 4.9 u at modifier 1.0 and 5.5 u at 1.3; the bound is 4 x 5.5 u = 22 u.  A transposed or mis-ordered T is
    off by the size of its entries (up to 1e3 here, i.e. > 1e6 u).  Returns T: the oracle is given these very bytes, because homographies
    that differ in their last bits move single gaussian_weights by more than stage A allows (a splat's weight is a difference of
    pixel-sized numbers)."""
    d = lambda k: torch.from_numpy(sc[k]).double()
    cov = RR.get_covariance_ref(d("means3D"), d("scales"), d("rotations"), modifier)
    want = RR.transmats_ref(cov, cam)
    ndc2pix = torch.tensor([[W / 2, 0, 0, (W - 1) / 2], [0, H / 2, 0, (H - 1) / 2], [0, 0, cam["zfar"] - cam["znear"], cam["znear"]], [0, 0, 0, 1]],
                           dtype=torch.float64).T
    col = (torch.from_numpy(cam["projmatrix"]).double() @ ndc2pix)[:, [0, 1, 3]].abs().sum(dim=0)
    unit = (cov[:, [0, 1, 3]].abs().amax(dim=2)[:, :, None] * col[None, None, :]).permute(0, 2, 1).reshape(-1, 9) * 2.0 ** -24
    assert T.shape == (P, 9) and T.dtype == np.float32
    assert _fig("D homographies, in units of u", float(((torch.from_numpy(T).double() - want).abs() / unit).max()), 22.0)
    return T


def _run_case(monkeypatch, fused, initial_stage=False, colour=False, scaling_modifier=1.0, compute_cov3D_python=False, depth_ratio=0.0,
              sh_degree=3, env_scope_center=(0.0, 0.0, 0.0), env_scope_radius=0.0):
    import gaussian_renderer as GR
    from oracle import oracle as orc
    monkeypatch.setattr(GR, "FUSED_REFLECTION", fused)
    sc, tex, fail, colours = _data()
    cam, View, PC, Pipe, t, bg = _setup(sh_degree, compute_cov3D_python, depth_ratio)
    handed = {}
    if compute_cov3D_python:
        host_side = GR._precomputed_transmats
        monkeypatch.setattr(GR, "_precomputed_transmats", lambda *a: handed.setdefault("T", host_side(*a)))
    pkg = GR.render(View, PC, Pipe, bg, scaling_modifier=scaling_modifier, override_color=t["colours"] if colour else None,
                    initial_stage=initial_stage, env_scope_center=list(env_scope_center), env_scope_radius=env_scope_radius)
    fused = fused and not initial_stage
    # ---- A
    kw = RR.raster_args(cam, sc, BG, sh_degree, scaling_modifier, colours if colour else None, env_scope_center, env_scope_radius,
                        compute_cov3D_python, dtype=np.float32)
    if compute_cov3D_python:
        kw["cov3D_precomp"] = _check_transmats(_npy(handed["T"]), sc, cam, scaling_modifier)
    o = orc.SurfelOracle(np.float32)
    fo = o.forward(**kw)
    allmap = _stage_a(pkg, fo, initial_stage)
    if env_scope_radius > 0:
        covered = allmap[1] > 0
        assert (allmap[7][covered] == 1).mean() > 0.1 and (allmap[7][covered] == 0).mean() > 0.1
    # ---- B
    base = _npy(pkg["render"] if initial_stage else pkg["base_color_map"])
    refl_map = np.zeros((1, H, W), np.float32) if initial_stage else _npy(pkg["refl_strength_map"])
    maps, leaves = RR.pixel_passes_ref(base, allmap, refl_map, tex, fail, cam, depth_ratio, initial_stage)
    _stage_b(pkg, maps, initial_stage)
    if compute_cov3D_python:
        # the quirk (tests/test_render_ref.py): no splat normal with a precomputed T, (0, 0, -1) instead; rend_normal is one constant vector,
        # scaled by A / (A + 1e-6) with A the blended weight, while the normal from depth still follows the surface
        assert float(np.abs(allmap[2:4]).max()) == 0.0 and float(allmap[4].max()) <= 0.0
        axis = -cam["viewmatrix"][:3, 2].astype(np.float64)
        A = -allmap[4].astype(np.float64)
        assert _fig("D rend_normal against the constant", float(np.abs(_npy(pkg["rend_normal"]) - axis[:, None, None] * (A / (A + 1e-6))[None]).max()), 2e-5)
        sn = _npy(pkg["surf_normal"])[:, allmap[1] > 0.5]
        assert float(sn.std(axis=1).max()) > 0.1
    # ---- C
    w = RR.make_weights(H, W, SEED + 1)
    with _captured(pkg, fused, initial_stage) as cap:
        RR.loss(pkg, w).backward()
    torch.cuda.synchronize()
    ref = RR.backward_ref(maps, leaves, w)
    zero = lambda *shape: np.zeros(shape, np.float32)
    g_base = _npy(cap["g_base"])
    g_s = _npy(cap["g_strength"]) if "g_strength" in cap else zero(1, H, W)
    planes = _npy(cap["allmap"]).copy()
    planes[2:5] += _npy(cap["g_normal_view"])
    bad = np.abs(planes[2:5] - ref["allmap"][2:5]).max(axis=0) > 1e-3 * np.abs(ref["allmap"][2:5]).max()
    ok = _fig("C pixel normal gradient, share of pixels", float(bad.mean()), 2e-3)
    ok &= _fig("C pixel base gradient", rel_maxnorm(g_base, ref["base"]), 1e-5)
    if not initial_stage:
        ok &= _fig("C pixel strength gradient", rel_maxnorm(g_s, ref["refl_map"]), 1e-4)
    for plane in (0, 1, 5, 6, 7):
        ok &= _fig("C pixel allmap[%d] gradient" % plane, rel_maxnorm(planes[plane], ref["allmap"][plane]), 1e-3)
    assert ok
    gr = o.backward(dL_dcolor=g_base, dL_dallmap=planes, dL_drefl_strength_map=g_s)
    want = {k: gr[ORACLE_NAMES[k]] for k in NAMES}
    if compute_cov3D_python:        # ---- D
        want.update(RR.python_path_gradients(sc, cam, scaling_modifier, gr["dL_dtransMat"], gr["dL_dmeans3D"]))
    ok, floors = True, (PYTHON_PATH_FLOOR if compute_cov3D_python else {})
    for k in NAMES:
        if k == "shs" and colour:
            assert t["shs"].grad is None
            ok &= _gate("override_color", _npy(t["colours"].grad), gr["dL_dcolors"])
            continue
        if compute_cov3D_python and k in ("means3D", "scales", "rotations"):
            print("FIG D %s smallest floor that passes %.3e" % (k, _needed_floor(_npy(t[k].grad), want[k])))
        ok &= _gate(k, _npy(t[k].grad), want[k], floors.get((k, scaling_modifier), 1e-6))
    if not colour:
        assert t["colours"].grad is None
    if compute_cov3D_python:
        print("FIG D viewspace_points smallest floor that passes %.3e" % _needed_floor(_npy(pkg["viewspace_points"].grad), gr["dL_dmeans2D"]))
    ok &= _gate("viewspace_points", _npy(pkg["viewspace_points"].grad), gr["dL_dmeans2D"], floors.get(("viewspace_points", scaling_modifier), 1e-6))
    if initial_stage:
        assert t["cubemap"].grad is None and t["fail"].grad is None
    else:
        ok &= _fig("C cubemap", rel_maxnorm(_npy(t["cubemap"].grad), ref["cubemap"]), 1e-4)
        ok &= _fig("C fail value", float(np.abs(_npy(t["fail"].grad) - ref["fail"]).max()), 1e-7 + 1e-5 * float(np.abs(ref["fail"]).max()))
    assert ok


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two-nodes"])
@pytest.mark.parametrize("case", list(CASES))
def test_render_option(case, fused, monkeypatch):
    _run_case(monkeypatch, fused, **CASES[case])


# --------------------------------------------------------------------------------------------- render_fast()
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two-nodes"])
@pytest.mark.parametrize("initial_stage", [False, True], ids=["full", "initial"])
@pytest.mark.parametrize("modifier", [0.7, 1.0, 1.6])
def test_render_fast_equals_render_at_every_modifier(modifier, initial_stage, fused, monkeypatch):
    """render_fast(), with autograd recording (the training forward) and under no_grad (the inference-only forward, which had only run at
    modifier 1), returns the bits of render() with the same modifier for every map both return; at 1.6 the inference-only forward's
    rasterizer planes are also held to the float32 oracle (stage A's bars)."""
    import gaussian_renderer as GR
    monkeypatch.setattr(GR, "FUSED_REFLECTION", fused)
    sc, tex, fail, _ = _data()
    cam, View, PC, Pipe, t, bg = _setup()
    full = GR.render(View, PC, Pipe, bg, scaling_modifier=modifier, initial_stage=initial_stage)
    keys = ("render", "rend_alpha", "rend_normal", "refl_strength_map") + (() if initial_stage else ("refl_color_map", "base_color_map"))
    for no_grad in (False, True):
        with torch.no_grad() if no_grad else torch.enable_grad():
            fast = GR.render_fast(View, PC, Pipe, bg, scaling_modifier=modifier, initial_stage=initial_stage)
        assert set(fast.keys()) == set(keys)
        assert fast["render"].requires_grad == (not no_grad)
        for k in keys:
            if k == "refl_strength_map" and initial_stage:
                continue                                    # render() does not return it in the initial stage
            assert torch.equal(fast[k], full[k]), (k, no_grad)
    if modifier == 1.6:
        from oracle import oracle as orc
        fo = orc.SurfelOracle(np.float32).forward(**RR.raster_args(cam, sc, BG, 3, modifier, dtype=np.float32))
        base = _npy(fast["render"] if initial_stage else fast["base_color_map"])
        assert psnr(base, fo["color"]) >= 50.0
        assert_image_close(base, fo["color"], 3e-5)
        assert psnr(_npy(fast["rend_alpha"]), fo["allmap"][1:2]) >= 50.0 and psnr(_npy(fast["refl_strength_map"]), fo["refl_strength_map"]) >= 50.0
        assert fo["num_rendered"] > 12000           # the modifier reached the kernel: 8903 instances at modifier 1 (tests/test_render_ref.py)


# --------------------------------------------------------------------------------------------- markVisible
NEAR = np.float32(0.2)
ULP = NEAR - np.nextafter(NEAR, np.float32(0))
# "rolled": the camera of every test above.  Its view matrix has 1.04 in the translation's z, so the float32 depth of a point near the near
# plane is the sum of two numbers of magnitude ~1 and lies on the grid of 2^-24, four times coarser than the floats around 0.2: 0.2f itself (an
# odd multiple of 2^-26) and its upper neighbour cannot come out, the lower neighbour can.  "rolled-z0": the same camera moved along its axis
# until that entry vanishes (eye . forward = 0: the eye's z solves z^2 - 5 z + 0.25 = 0), where the depth is a sum at the magnitude of 0.2 and
# all three values come out.
MARK_CAMERAS = {"rolled": (0.4, -0.3, -1.0), "rolled-z0": (0.4, -0.3, 2.5 - np.sqrt(6.0))}


def _view_depth(m, pts):
    """Float32 view depth in the kernel's order (csrc/gsr_common.hip mark_visible_kernel and the oracle's transformPoint4x3, contraction off)."""
    m, f = m.astype(np.float32), np.float32
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return f(f(f(f(m[0, 2] * x) + f(m[1, 2] * y)) + f(m[2, 2] * z)) + m[3, 2])


def _near_plane_points(n, view, rs):
    """Up to n world points (float32) AT the near plane of the frustum test: aimed in view space at depth 0.2f, one float32 ulp below and one
    above in turn, mapped back with the float64 inverse, rounded, and kept only where the float32 recomputation lands within 4 ulps of 0.2f
    (a few draws per slot).  Returns (points, their recomputed depths)."""
    inv = np.linalg.inv(view.astype(np.float64))
    pts = []
    for slot in range(n):
        target = float(NEAR) + (slot % 3 - 1) * float(ULP)
        for _ in range(16):
            p = (np.array([rs.uniform(-0.1, 0.1), rs.uniform(-0.1, 0.1), target, 1.0]) @ inv)[:3].astype(np.float32)
            if abs(float(_view_depth(view, p[None])[0]) - float(NEAR)) <= 4 * float(ULP):
                pts.append(p)
                break
    pts = np.array(pts, np.float32).reshape(-1, 3)
    return pts, _view_depth(view, pts)


@pytest.mark.parametrize("variant", ["surfel", "gauss"])
@pytest.mark.parametrize("camera", list(MARK_CAMERAS))
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3000])
def test_mark_visible_equals_oracle(n, camera, variant):
    """GaussianRasterizer.markVisible of both packages, through the ctypes binding and, where it is built, the compiled one, at point counts
    around the kernel's block of 256, under the rolled camera, against oracle.mark_visible: exactly equal.  A tenth of the points sit at the
    near plane of the frustum test (view depth <= 0.2 is out: in_frustum, DSR auxiliary.h).  At n = 3000, under "rolled-z0" at least 20 of
    them must have landed exactly on 0.2f, 20 exactly one float32 ulp nearer and 20 exactly one farther; under "rolled" (see MARK_CAMERAS:
    0.2f itself is out of that camera's reach) at least 20 within 4 ulps on either side."""
    import _gsr
    from oracle import oracle as orc
    if variant == "surfel":
        from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
        extra = {}
    else:
        from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
        extra = {"antialiasing": False}
    cam = S.look_at_camera(W, H, eye=MARK_CAMERAS[camera], target=(0, 0, 5))
    rs = np.random.RandomState(n)
    pts = _data()[0]["means3D"][:n].copy()
    edge, depth = _near_plane_points(n // 10, cam["viewmatrix"], rs)
    pts[:len(edge)] = edge
    if n == 3000 and camera == "rolled-z0":
        assert abs(float(cam["viewmatrix"][3, 2])) < 1e-6
        counts = [(depth == NEAR - ULP).sum(), (depth == NEAR).sum(), (depth == NEAR + ULP).sum()]
        assert min(counts) >= 20, counts
    elif n == 3000:
        assert (depth < NEAR).sum() >= 20 and (depth > NEAR).sum() >= 20, ((depth < NEAR).sum(), (depth > NEAR).sum())
    want = orc.mark_visible(pts, cam["viewmatrix"], cam["projmatrix"])
    np.testing.assert_array_equal(want[:len(edge)], depth > NEAR)          # the oracle itself puts the boundary where intended
    if n == 3000:
        assert 0.5 < want.mean() < 1.0                  # make_scene's near-cull subset is out, the box is in
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.zeros(3, device="cuda"),
                                       scale_modifier=1.0, viewmatrix=c(cam["viewmatrix"]), projmatrix=c(cam["projmatrix"]), sh_degree=3,
                                       campos=c(cam["campos"]), prefiltered=False, debug=False, **extra)
    compiled = _gsr.PYBIND
    try:
        for binding in (None, compiled) if compiled is not None else (None,):
            _gsr.PYBIND = binding
            got = GaussianRasterizer(st).markVisible(c(pts))
            assert got.dtype == torch.bool and got.shape == (n,)
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg="compiled" if binding is not None else "ctypes")
    finally:
        _gsr.PYBIND = compiled
