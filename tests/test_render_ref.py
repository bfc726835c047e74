"""Pins of tests/render_ref.py, the checker tests/test_gpu_render_options.py compares render() / render_fast() with (CPU only).

The checker is composed from the oracle and the float64 chains, which have their own pins; what is new in it is the reference's host side
(get_covariance, the Python homographies, the env-scope sphere) and the loss.  They are pinned here against the oracle itself: the two routes
to a homography must agree, the gradient through the Python route must agree with finite differences, and the scenes of the GPU test must
reach the branches they are there for."""
import numpy as np
import pytest
import torch

import render_ref as RR
from helpers import S

# the scene of tests/test_gpu_render_options.py
P, W, H, L, SEED, MU = 3000, 200, 136, 16, 5, -2.8
BG = (0.1, 0.2, 0.3)
SCOPE = dict(env_scope_center=(0.5, 0.2, 5.0), env_scope_radius=1.6)


def _camera(w=W, h=H):
    return S.look_at_camera(w, h, eye=(0.4, -0.3, -1.0), target=(0, 0, 5))


@pytest.fixture(scope="module")
def scene():
    sc = S.make_scene(P, "S", seed=SEED, mu=MU)
    tex, fail = S.make_cubemap(L, 3, SEED)
    return sc, tex, fail


@pytest.mark.parametrize("modifier", [1.0, 1.3])
def test_python_homographies_reproduce_the_rasterizers_own(scene, modifier):
    """The float64 oracle fed transmats_ref(get_covariance_ref(...)) as cov3D_precomp against the float64 oracle fed scales and rotations
    (compute_transmat, DSR forward.cu:30-66), scaling modifier included.  Measured at modifier 1.0 / 1.3: colour max-abs 7.8e-14 / 5.8e-14,
    alpha 1.0e-13 / 6.1e-14, reflection strength 7.1e-15 / 5.2e-15, distortion 9.0e-16 / 7.2e-16, and on the two depth planes, whose values
    reach 166 and 374 (an edge-on splat just behind the near plane), 8.5e-10 / 1.1e-9 and 1.9e-9 / 1.1e-11 absolute, i.e. <= 1e-11 of the
    plane's peak.  The bound is 1e-9 of the plane's own peak, the peak taken as at least 1 (the convention of helpers.assert_planes_psnr): a
    wrong row or column order, a missing modifier or a (W-1)/2 slip shows at 1e-2 or more.

    The quirk: with a precomputed T the rasterizer does not know the splat's normal and sets it to (0, 0, 1), flipped towards the camera
    (DSR forward.cu:200-215); the oracle does the same.  So the blended normal planes allmap[2:5] of the two paths DIFFER, by about 1, and
    the precomputed path's x and y planes are exactly zero ("currently don't support normal consistency loss if use precomputed covariance",
    gaussian_renderer/__init__.py:96 of the reference)."""
    sc, tex, fail = scene
    cam = _camera()
    a = RR.render_ref(cam, sc, tex, fail, BG, scaling_modifier=modifier).raster
    b = RR.render_ref(cam, sc, tex, fail, BG, scaling_modifier=modifier, compute_cov3D_python=True).raster
    assert a["num_rendered"] == b["num_rendered"] > 0
    np.testing.assert_array_equal(a["radii"], b["radii"])
    pairs = [("color", a["color"], b["color"]), ("refl_strength_map", a["refl_strength_map"], b["refl_strength_map"])]
    pairs += [("allmap[%d]" % p, a["allmap"][p], b["allmap"][p]) for p in (0, 1, 5, 6)]
    for name, x, y in pairs:
        err, peak = float(np.abs(x - y).max()), max(1.0, float(np.abs(x).max()))
        print(name, modifier, err, peak)
        assert err <= 1e-9 * peak, (name, err, peak)
    assert float(np.abs(a["allmap"][2:5] - b["allmap"][2:5]).max()) > 0.5
    assert float(np.abs(b["allmap"][2:4]).max()) == 0.0 and float(b["allmap"][4].min()) < -0.5 and float(b["allmap"][4].max()) <= 0.0
    assert float(np.abs(a["allmap"][2:4]).max()) > 0.5


def test_key_sets_are_the_references():
    sc = S.make_scene(50, "S", seed=3, mu=-1.5)
    tex, fail = S.make_cubemap(4, 3, 3)
    cam = _camera(32, 24)
    full = RR.render_ref(cam, sc, tex, fail, BG)
    first = RR.render_ref(cam, sc, tex, fail, BG, initial_stage=True)
    # gaussian_renderer/__init__.py:202-217 and :183-195 of the reference
    assert set(full.keys()) == {"render", "viewspace_points", "visibility_filter", "radii", "rend_alpha", "rend_normal", "rend_dist", "surf_depth",
                                "surf_normal", "env_scope_mask", "refl_strength_map", "refl_color_map", "base_color_map", "gaussian_weights"}
    assert set(first.keys()) == {"render", "viewspace_points", "visibility_filter", "radii", "rend_alpha", "rend_normal", "rend_dist", "surf_depth",
                                 "surf_normal", "gaussian_weights", "env_scope_mask"}
    assert set(full.keys()) == RR.KEYS_FULL and set(first.keys()) == RR.KEYS_INITIAL
    assert full["render"].shape == (3, 24, 32) and first["render"] is first.leaves["base"]
    # the loss reaches every map it names, in both stages
    w = RR.make_weights(24, 32, 1)
    for pkg in (full, first):
        g = RR.backward_ref(pkg, pkg.leaves, w)
        assert np.abs(g["base"]).max() > 0 and all(np.abs(g["allmap"][p]).max() > 0 for p in (0, 1, 2, 3, 4, 6))
        assert (np.abs(g["cubemap"]).max() > 0) == (pkg is full) and (np.abs(g["refl_map"]).max() > 0) == (pkg is full)


def test_env_scope_mask_is_the_strict_inside_of_the_sphere():
    xyz = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0, 0, 5], [3, 4, 0], [3, 4, 1e-3]], dtype=np.float64)
    assert list(RR.env_scope_mask_ref(xyz, (0, 0, 0), 5.0)) == [True, True, True, False, False, False]      # `<`: the surface is outside
    assert list(RR.env_scope_mask_ref(xyz, (3, 4, 0), 1.0)) == [False, False, False, False, True, True]
    assert RR.env_scope_mask_ref(xyz, (3, 4, 0), 0.0).all() and RR.env_scope_mask_ref(xyz, (3, 4, 0), 0.0).shape == (6,)


def test_get_covariance_ref_known_answer():
    """Identity rotation given as a quaternion of length 2, scales (2, 3), modifier 0.5, centre (7, 8, 9): rows = tangent axes times the
    modified scales, the normal, the centre (scene/gaussian_model.py:34-40); then a quarter turn about z, which sends the first tangent to +y."""
    xyz = torch.tensor([[7.0, 8.0, 9.0]] * 2, dtype=torch.float64)
    q = torch.tensor([[2.0, 0, 0, 0], [np.sqrt(0.5) * 3, 0, 0, np.sqrt(0.5) * 3]], dtype=torch.float64)
    cov = RR.get_covariance_ref(xyz, torch.tensor([[2.0, 3.0]] * 2, dtype=torch.float64), q, 0.5)
    np.testing.assert_allclose(cov[0].numpy(), [[1, 0, 0, 0], [0, 1.5, 0, 0], [0, 0, 1, 0], [7, 8, 9, 1]], atol=1e-15)
    np.testing.assert_allclose(cov[1].numpy(), [[0, 1, 0, 0], [-1.5, 0, 0, 0], [0, 0, 1, 0], [7, 8, 9, 1]], atol=1e-15)


# --------------------------------------------------------------------------------------------- gradient through the Python path
FD_P, FD_W, FD_H = 200, 64, 48


def _fd_scene():
    """Near face-on surfels a few pixels across, as in test_oracle_fd.test_surfel_depth_and_distortion_gradient_fd_ray_splat_branch: in the
    low-pass branch the reference's backward holds the intersection point constant (tests/test_oracle_quirks.py), so depth, distortion and the
    normal from depth are true gradients only where the ray-splat branch is taken.  The quaternions are RAW (lengths 0.5 to 2)."""
    rs = np.random.RandomState(11)
    sc = {k: v.astype(np.float64) for k, v in S.make_scene(FD_P, "S", seed=11, mu=-1.0, cull_frac=0.0).items() if k != "env_scope_mask"}
    sc["scales"] = np.exp(rs.normal(-1.0, 0.2, (FD_P, 2)))
    q = np.concatenate([np.ones((FD_P, 1)), 0.12 * rs.normal(size=(FD_P, 3))], axis=1)
    sc["rotations"] = q / np.linalg.norm(q, axis=1, keepdims=True) * rs.uniform(0.5, 2.0, (FD_P, 1))
    sc["opacities"] = np.clip(sc["opacities"], 0.05, 0.9)
    return sc


def test_gradient_through_the_python_homographies_matches_finite_differences():
    """pipe.compute_cov3D_python at modifier 1.0, all in float64: the oracle's dL_dtransMat pulled back through autograd of
    transmats_ref o get_covariance_ref, plus the oracle's direct dL_dmeans3D (render_ref.python_path_gradients), against central differences of
    loss(render_ref(...)) (step 1e-6, tolerance 5e-5 of the largest difference of the tensor: test_oracle_fd's for the surfel variant) on
    seven entries each of position, scale and raw quaternion of visible splats.  The loss jumps where a step changes a radius, a contributor
    count or the side of the alpha >= 1/255 test of a pair: an entry is skipped when a radius or a count changes, or when the second
    difference L(+) + L(-) - 2 L(0) exceeds 1e-3 of L(+) - L(-) (for a smooth loss it is ~1e-6 of it; a jump makes it as large); at least
    five of each kind must remain.  The reference multiplies surf_normal by the DETACHED alpha (gaussian_renderer/__init__.py:176), so the
    differences are taken with that factor held at its unperturbed value.  The raw quaternion's gradient is a TRUE gradient on this path: the
    normalisation is torch's, not the rasterizer's un-projected quat_to_rotmat_vjp (test_oracle_fd.test_surfel_rotation_gradient_fd)."""
    sc = _fd_scene()
    tex, fail = S.make_cubemap(8, 3, 11)
    tex, fail = tex.astype(np.float64), fail.astype(np.float64)
    cam = _camera(FD_W, FD_H)
    w = RR.make_weights(FD_H, FD_W, 12)

    def run(s):
        return RR.render_ref(cam, s, tex, fail, BG, compute_cov3D_python=True, **SCOPE)
    pkg = run(sc)
    radii, nc = pkg.raster["radii"].copy(), pkg.oracle.state("n_contrib").copy()
    alpha0 = pkg["rend_alpha"].detach().clone()

    def detached_alpha(p):
        """p with surf_normal = (normal from depth) * alpha0 instead of * its own alpha."""
        a = p["rend_alpha"].detach()
        q = dict(p)
        q["surf_normal"] = torch.where(a > 0, p["surf_normal"] / torch.where(a > 0, a, torch.ones_like(a)) * alpha0, p["surf_normal"])
        return q
    assert pkg.raster["num_rendered"] > 0 and 0.1 < pkg.raster["allmap"][7].mean() < 0.9
    loss0 = float(RR.loss(pkg, w).detach())
    g = RR.backward_ref(pkg, pkg.leaves, w)
    gr = pkg.oracle.backward(dL_dcolor=g["base"], dL_dallmap=g["allmap"], dL_drefl_strength_map=g["refl_map"])
    analytic = RR.python_path_gradients(sc, cam, 1.0, gr["dL_dtransMat"], gr["dL_dmeans3D"])
    rs = np.random.RandomState(13)
    splats = rs.choice(np.nonzero(radii > 0)[0], 7, replace=False)
    eps = 1e-6
    for key in ("means3D", "scales", "rotations"):
        fd, an = [], []
        for i in splats:
            c = rs.randint(sc[key].shape[1])
            vals, same = [], True
            for sign in (1.0, -1.0):
                q = {k: v.copy() for k, v in sc.items()}
                q[key][i, c] += sign * eps
                p = run(q)
                same = same and (p.raster["radii"] == radii).all() and (p.oracle.state("n_contrib") == nc).all()
                vals.append(float(RR.loss(detached_alpha(p), w).detach()))
            if same and abs(vals[0] + vals[1] - 2 * loss0) <= 1e-3 * abs(vals[0] - vals[1]) + 1e-14:
                fd.append((vals[0] - vals[1]) / (2 * eps))
                an.append(analytic[key][i, c])
        fd, an = np.array(fd), np.array(an)
        print(key, len(fd), np.abs(fd - an).max() / np.abs(fd).max())
        assert len(fd) >= 5, key
        assert np.abs(fd - an).max() <= 5e-5 * np.abs(fd).max(), (key, fd, an)


# --------------------------------------------------------------------------------------------- reach of the GPU test's scenes
def test_gpu_scenes_reach_what_they_claim(scene):
    """Float32 oracle on the scene of tests/test_gpu_render_options.py.  Measured: 1228 splats inside the env-scope sphere and 1772 outside; the
    mask plane is 1 at 31 % and 0 at 69 % of the covered pixels; 32 % of the pixels are empty; modifiers 0.7 / 1.0 / 1.6 render 6827 / 8903 /
    14212 instances."""
    sc, tex, fail = scene
    cam = _camera()
    assert abs(cam["FoVx"] - cam["FoVy"]) > 0.1 and abs(cam["viewmatrix"][0, 1]) > 1e-3          # FoVx != FoVy, rolled
    inside = RR.env_scope_mask_ref(sc["means3D"], SCOPE["env_scope_center"], SCOPE["env_scope_radius"])
    assert inside.sum() > 500 and (~inside).sum() > 500
    fo = RR.render_ref(cam, sc, tex, fail, BG, dtype=np.float32, **SCOPE).raster
    alpha, mask = fo["allmap"][1], fo["allmap"][7]
    covered = alpha > 0
    assert set(np.unique(mask)) == {0.0, 1.0}
    assert (mask[covered] == 1).mean() > 0.10 and (mask[covered] == 0).mean() > 0.10
    assert (alpha == 0).mean() > 0.05
    n = [RR.render_ref(cam, sc, tex, fail, BG, scaling_modifier=m, dtype=np.float32).raster["num_rendered"] for m in (0.7, 1.0, 1.6)]
    assert 0 < n[0] < n[1] < n[2], n
    # without a radius every covered pixel is inside the scope
    full = RR.render_ref(cam, sc, tex, fail, BG, dtype=np.float32).raster["allmap"]
    assert (full[7][full[1] > 0] == 1).all()
