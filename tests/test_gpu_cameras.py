"""GPU: both rasterizers under the camera families of tests/cameras.py (fx != fy, off-centre principal point, rolled pose, narrow and
wide FoV, image sizes at which the surfel backward rebuilds its homography for W - 1 and H - 1, and all of these at once), against the
float32 oracle at the bars of tests/test_gpu_parity.py, unchanged:
  * num_rendered, radii and the binning state (test_gpu_parity._check_binning) exact, n_contrib within N_CONTRIB_BUDGET;
  * images within assert_image_close at 3e-5 (S) / 5e-4 (G), every plane at PSNR >= 50 dB;
  * every gradient tensor within rel_maxnorm <= 1e-4 and grad_gate <= GATE_BUDGET;
  * variant G: the same two gradient checks once more on the VISIBLE rows whose view-space position lies beyond 1.3 x the FoV (the
    frustum clamp of the projection Jacobian), so that those few hundred rows cannot hide in the budget of the whole tensor.
One family misses a bar without the kernels being at fault, variant G under `wide`; what it gets instead is derived from the float32
oracle's own distance to the float64 oracle on that scene (GATE_FLOOR, MAXNORM_BAR below).
tests/test_cameras_host.py proves on the CPU that every family reaches what it was built for; tests/test_oracle_dense.py and
tests/test_oracle_quirks.py pin the oracle under such cameras first.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import cameras as C
from helpers import GATE_BUDGET, HipGauss, HipSurfel, S, assert_image_close, assert_planes_psnr, grad_gate, n_contrib_ok, psnr, rel_maxnorm
from test_gpu_parity import GRAD_TOL, PSNR_MIN, _check_binning, _oracle

pytestmark = pytest.mark.gpu

S_GRADS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_drefl_strengths", "dL_dscales", "dL_drotations")
G_GRADS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dnormals", "dL_drefl_strengths", "dL_dscales", "dL_drotations")


# The elementwise gate's floor (helpers.grad_gate: |a - b| <= 1e-4 |b| + floor * max|b|) is 1e-6 everywhere but for variant G under `wide`.
# There the float32 ORACLE, measured on the CPU against the float64 oracle on that very scene (same inputs, same upstream gradients),
# needs a floor of 8.5e-7 for dL_dmeans3D, 6.1e-6 for dL_dmeans2D, 2.5e-6 for dL_dscales and 2.8e-6 for dL_drotations to leave no element
# out: at 110 degrees the projection Jacobian of the clamped Gaussians has entries of 2.7 x the focal length, and the small elements of
# these four tensors are differences of such products.  Floor = 4 x that measurement (the project's margin for summation order), and
# never more than the 1e-5 tests/test_gpu_random_sweep.py uses; rtol, GATE_BUDGET and the 1e-4 of rel_maxnorm stay.  What the GPU needs is
# printed ("needs floor").
# The clamped visible rows of that scene, taken alone (489 rows, judged against THEIR maximum, 1.9 % of the tensor's for dL_dmeans3D):
# the float32 oracle is 5.5e-5 / 5.6e-5 / 4.0e-5 of that maximum away from the float64 oracle in dL_dmeans3D / dL_dscales /
# dL_drotations and needs floors of 3.0e-5 / 8.8e-6 / 1.1e-5 (dL_dopacity: 3.4e-6 and 2.1e-8, it keeps both bars).  Two float32
# evaluations that far from the truth cannot agree to 1e-4 and 1e-6 with each other; the bars of these three become the larger of
# the existing bar and 4 x the measurement, both for rel_maxnorm and for the floor.  No other family needs either.
GATE_FLOOR = {"wide G": dict(dL_dmeans3D=4 * 8.5e-7, dL_dmeans2D=1e-5, dL_dscales=4 * 2.5e-6, dL_drotations=1e-5),
              "wide G clamped": dict(dL_dmeans3D=4 * 3.0e-5, dL_dscales=4 * 8.8e-6, dL_drotations=4 * 1.1e-5)}
MAXNORM_BAR = {"wide G clamped": dict(dL_dmeans3D=4 * 5.5e-5, dL_dscales=4 * 5.6e-5, dL_drotations=4 * 4.0e-5)}


def _needed_floor(a, b):
    """The smallest floor with which helpers.grad_gate(a, b) stays within GATE_BUDGET."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    need = np.sort((np.abs(a - b) - GRAD_TOL * np.abs(b)) / max(float(np.abs(b).max()), 1e-300))[::-1]
    return max(float(need[int(GATE_BUDGET * a.size)]), 0.0)


def _check_grads(gh, gr, keys, what, rows=None, floors=None, bars=None):
    """rel_maxnorm <= GRAD_TOL and grad_gate <= GATE_BUDGET on every tensor of `keys` (on `rows` of it alone where given)."""
    fails = []
    for k in keys:
        a, b = gh[k].reshape(gr[k].shape), gr[k]
        if rows is not None:
            a, b = a[rows], b[rows]
        floor, bar = (floors or {}).get(k, 1e-6), max(GRAD_TOL, (bars or {}).get(k, 0.0))
        err, bad = rel_maxnorm(a, b), grad_gate(a, b, GRAD_TOL, floor)
        print(f"{what} {k}: rel_maxnorm {err:.2e} (bar {bar:.1e}) gate {bad:.2e} at floor {floor:.1e}, needs floor {_needed_floor(a, b):.2e} "
              f"({a.shape[0]} rows, max {np.abs(b).max():.2e})")
        if not np.isfinite(a).all() or err > bar or bad > GATE_BUDGET:
            fails.append((what, k, err, bad))
    assert not fails, fails


def check_surfel(kw, seed, what, keys=S_GRADS, check_binning=_check_binning):
    """Variant S against the float32 oracle with the checks of test_gpu_parity._run_surfel; returns (hip gradients, oracle gradients)."""
    H, W = kw["image_height"], kw["image_width"]
    o = _oracle().SurfelOracle(np.float32)
    ref = o.forward(**kw)
    hip = HipSurfel(kw)
    out = hip.out()
    assert out["num_rendered"] == ref["num_rendered"] > 0
    np.testing.assert_array_equal(out["radii"], ref["radii"])
    check_binning(hip, o)
    nc_h, nc_o = hip.state("n_contrib").astype(np.uint32), o.state("n_contrib")
    print(f"{what}: R {ref['num_rendered']} n_contrib off {(nc_h != nc_o).sum()} colour {np.abs(out['color'] - ref['color']).max():.2e}")
    assert n_contrib_ok(nc_h[0], nc_o[0]) and n_contrib_ok(nc_h[1], nc_o[1])
    assert psnr(out["color"], ref["color"]) >= PSNR_MIN
    assert_image_close(out["color"], ref["color"], 3e-5)
    assert psnr(out["refl_strength_map"], ref["refl_strength_map"]) >= PSNR_MIN
    assert_planes_psnr(out["allmap"], ref["allmap"], PSNR_MIN)
    gw_h, gw_o = out["gaussian_weights"].astype(np.float64), ref["gaussian_weights"].astype(np.float64)
    gw_bad = np.abs(gw_h - gw_o) > 1.5e-6 + 1e-5 * np.abs(gw_o)
    assert int(gw_bad.sum()) <= max(2, int(3e-5 * gw_o.size)) and np.abs(gw_h - gw_o).max() <= 5e-3, (int(gw_bad.sum()), np.abs(gw_h - gw_o).max())
    g = S.make_upstream_grads(H, W, seed)
    gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dallmap=g["dL_dplanes"], dL_drefl_strength_map=g["dL_drefl"])
    gh = hip.backward(g["dL_dcolor"], g["dL_dplanes"], g["dL_drefl"])
    _check_grads(gh, gr, keys, what)
    return gh, gr


def check_gauss(kw, seed, antialiasing, what):
    """Variant G against the float32 oracle with the checks of test_gpu_parity._run_gauss, then the gradient checks again on the visible
    frustum-clamped rows alone."""
    H, W = kw["image_height"], kw["image_width"]
    o = _oracle().GaussOracle(np.float32)
    ref = o.forward(antialiasing=antialiasing, **kw)
    hip = HipGauss(kw, antialiasing=antialiasing)
    out = hip.out()
    assert out["num_rendered"] == ref["num_rendered"] > 0
    np.testing.assert_array_equal(out["radii"], ref["radii"])
    _check_binning(hip, o)
    nc_h, nc_o = hip.state("n_contrib").astype(np.uint32)[0], o.state("n_contrib")
    print(f"{what}: R {ref['num_rendered']} n_contrib off {(nc_h != nc_o).sum()} colour {np.abs(out['color'] - ref['color']).max():.2e}")
    assert n_contrib_ok(nc_h, nc_o)
    for k in ("color", "normal_map", "refl_strength_map", "invdepth"):
        assert psnr(out[k], ref[k], peak=max(1.0, float(np.abs(ref[k]).max()))) >= PSNR_MIN, k
    assert_image_close(out["color"], ref["color"], 5e-4)
    g = S.make_upstream_grads(H, W, seed)
    gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dinvdepth=g["dL_dinvdepth"], dL_dnormal_map=g["dL_dnormal"], dL_drefl_strength_map=g["dL_drefl"])
    gh = hip.backward(g["dL_dcolor"], g["dL_dinvdepth"], g["dL_dnormal"], g["dL_drefl"])
    floors = GATE_FLOOR.get(" ".join(what.split()[:2]))
    _check_grads(gh, gr, G_GRADS, what, floors=floors)
    cx, cy = C.clamp_classes(kw)
    clamped = (cx | cy) & (ref["radii"] > 0)
    assert clamped.sum() >= 100 and np.abs(gr["dL_dmeans3D"][clamped]).max() > 0
    _check_grads(gh, gr, ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity"), what + " clamped rows", rows=clamped,
                 floors=GATE_FLOOR.get(" ".join(what.split()[:2]) + " clamped"), bars=MAXNORM_BAR.get(" ".join(what.split()[:2]) + " clamped"))
    return gh, gr


# ------------------------------------------------------------------------------------------- every family, both variants
@pytest.mark.parametrize("name", C.FAMILIES)
def test_surfel_under_camera_family(name):
    kw, _ = C.scene(name, "S")
    check_surfel(kw, C.SEEDS[name], name + " S")


# anti-aliasing alternates over the families: on for four of them ("all" among them), off for three
@pytest.mark.parametrize("name,antialiasing", [(n, i % 2 == 0) for i, n in enumerate(C.FAMILIES)])
def test_gauss_under_camera_family(name, antialiasing):
    kw, _ = C.scene(name, "G")
    check_gauss(kw, C.SEEDS[name], antialiasing, f"{name} G aa={int(antialiasing)}")


def test_surfel_truncating_camera_and_its_sibling_differ_by_the_truncation_alone():
    """trunc_x has the fy of trunc moved by a few ulps, to where int(focal_y * tan_fovy * 2) is H and not H - 1: the same scene, forwards
    equal to rounding.  Both pass against their own oracle run, and the two HIP gradient sets differ by more than 1e-3 in dL_dscales —
    the Hb / H the backward's homography is rebuilt with — so a kernel that ignored the truncation, or truncated always, fails one of them."""
    kw, kw_x, cam = C.trunc_pair()
    gh, _ = check_surfel(kw, C.SEEDS["trunc"], "trunc S")
    gh_x, _ = check_surfel(kw_x, C.SEEDS["trunc"], "trunc_x S")
    diff = rel_maxnorm(gh_x["dL_dscales"], gh["dL_dscales"])
    print(f"trunc against trunc_x, dL_dscales: {diff:.2e} (1 / H = {1 / cam['H']:.2e})")
    assert 1e-3 < diff < 10.0 / cam["H"]


def test_surfel_precomputed_homographies_under_all():
    """cov3D_precomp (the backward's `precomp` path: no rebuild of T, dL_dtransMat returned) with the oracle's own homographies."""
    kw, _ = C.scene("all", "S")
    o = _oracle().SurfelOracle(np.float32)
    o.forward(**kw)
    T = o.state("transMat").reshape(-1, 9).copy()
    T[o.state("radii") == 0] = np.eye(3, dtype=np.float32).reshape(-1)        # culled surfels never wrote their T
    kw = dict(kw, cov3D_precomp=np.ascontiguousarray(T), scales=None, rotations=None)
    check_surfel(kw, 71, "all S precomp", keys=S_GRADS[:5] + ("dL_dtransMat",))


def test_surfel_precomputed_colours_under_all():
    """colors_precomp: no SH pass, so the SH clamp flags (the last comparison of _check_binning) are written by nobody; the binning
    state is compared with test_gpu_adversarial.check_binning, which is _check_binning without them."""
    from test_gpu_adversarial import check_binning
    kw, _ = C.scene("all", "S")
    kw = dict(kw, colors_precomp=np.random.RandomState(72).rand(kw["means3D"].shape[0], 3).astype(np.float32), shs=None)
    check_surfel(kw, 72, "all S colours", check_binning=check_binning,
                 keys=("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dcolors", "dL_drefl_strengths", "dL_dscales", "dL_drotations"))


@pytest.mark.parametrize("refl", [False, True])
def test_eval_forward_is_bit_identical_under_all(refl):
    """test_gpu_eval_forward's comparison (every plane of the inference forward the same bits as the training forward's) under `all`."""
    from test_gpu_eval_forward import _compare
    kw, cam = C.scene("all", "S")
    v = C.view_of(cam)
    t = {k: torch.from_numpy(kw[k]).cuda() for k in ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")}
    t["colors"] = t["transmat"] = None
    tex, fail = S.make_cubemap(16, 3, 73)
    s = dict(t=t, cam=cam, ct=v.ct, W=cam["W"], H=cam["H"], degree=3, cubemap=torch.from_numpy(tex).cuda(),
             fail=torch.from_numpy(fail).cuda() + 0.25, bg=torch.tensor([0.1, 0.2, 0.3], device="cuda"))
    n, others = _compare(s, refl)
    assert n > 0 and float(others[1].max()) > 0.5


@pytest.mark.parametrize("name", ["rolled", "offcentre"])
@pytest.mark.parametrize("variant", ["surfel", "gauss"])
def test_mark_visible_under_camera_family(name, variant):
    from oracle import oracle as orc
    if variant == "surfel":
        from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
        extra = {}
    else:
        from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
        extra = {"antialiasing": False}
    kw, cam = C.scene(name, "S")
    want = orc.mark_visible(kw["means3D"], cam["viewmatrix"], cam["projmatrix"])
    assert 0.5 < want.mean() < 1.0 - 0.5 * C.NEAR_FRAC
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = GaussianRasterizationSettings(image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                       bg=torch.zeros(3, device="cuda"), scale_modifier=1.0, viewmatrix=c(cam["viewmatrix"]),
                                       projmatrix=c(cam["projmatrix"]), sh_degree=3, campos=c(cam["campos"]), prefiltered=False, debug=False, **extra)
    got = GaussianRasterizer(st).markVisible(c(kw["means3D"]))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
