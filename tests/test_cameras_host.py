"""CPU: the camera builder of tests/cameras.py against the reference's own matrices (tests/golden/camera_hwk_golden.npz), and every
camera family reaching what it was built for, measured on the float32 oracle.  A family that misses its target tests nothing on the GPU.
The scenes are the ones tests/test_gpu_cameras.py renders (cameras.scene: same family, size and seed).  These are conditions, not
measurements: the seeds in cameras.SEEDS are fixed so that they hold."""
import os

import numpy as np
import pytest

import cameras as C
from oracle import oracle as orc

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_hwk_camera_matches_reference_graphics_utils():
    g = np.load(os.path.join(G, "camera_hwk_golden.npz"))
    assert int(g["n"]) >= 6
    for i in range(int(g["n"])):
        W, H, fx, fy, cx, cy = g[f"hwk{i}"]
        assert abs(fx / fy - 1) > 0.2 and abs(cx - W / 2) > 0.09 * W and abs(cy - H / 2) > 0.09 * H
        cam = C.hwk_camera(int(W), int(H), fx, fy, cx, cy, R=g[f"R{i}"], T=g[f"T{i}"])
        np.testing.assert_allclose([cam["FoVx"], cam["FoVy"]], g[f"fov{i}"], rtol=1e-12)
        np.testing.assert_allclose([cam["tanfovx"], cam["tanfovy"]], np.tan(0.5 * g[f"fov{i}"]), rtol=1e-12)
        np.testing.assert_allclose(cam["viewmatrix"], g[f"wvt{i}"], atol=1e-6)
        np.testing.assert_allclose(cam["projmatrix"], g[f"full{i}"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(cam["campos"], g[f"center{i}"], atol=2e-5)
        # the projection alone: full = view @ proj with an invertible view
        proj = np.linalg.inv(cam["viewmatrix"].astype(np.float64)) @ cam["projmatrix"].astype(np.float64)
        np.testing.assert_allclose(proj, g[f"projc{i}"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(cam["K"], [[fx, 0, cx], [0, fy, cy], [0, 0, 1]], rtol=1e-6)


def test_hwk_camera_with_centred_square_pixels_is_make_camera():
    a = C.S.make_camera(200, 136)
    b = C.hwk_camera(200, 136, a["K"][0, 0], a["K"][1, 1], 100.0, 68.0)
    for k in ("viewmatrix", "projmatrix", "campos", "K"):
        np.testing.assert_allclose(b[k], a[k], rtol=1e-6, atol=1e-7, err_msg=k)
    np.testing.assert_allclose([b["tanfovx"], b["tanfovy"]], [a["tanfovx"], a["tanfovy"]], rtol=1e-6)


# ------------------------------------------------------------------------------------------- what each family is
def _bsize(cam):
    return C.backward_size(cam["W"], cam["tanfovx"]), C.backward_size(cam["H"], cam["tanfovy"])


def _is_aniso(cam):
    r = float(cam["K"][0, 0] / cam["K"][1, 1])
    return 1.25 < max(r, 1 / r) < 1.55


def _is_offcentre(cam):
    dx, dy = abs(cam["K"][0, 2] - cam["W"] / 2) / cam["W"], abs(cam["K"][1, 2] - cam["H"] / 2) / cam["H"]
    return 0.1 <= dx <= 0.2 and 0.1 <= dy <= 0.2


def _is_rolled(cam):
    V = cam["viewmatrix"].astype(np.float64)
    blocks = [V[i:i + 3, j:j + 3] for i in (0, 1) for j in (0, 1)]
    return all(np.abs(b - b.T).max() > 0.1 for b in blocks) and np.abs(cam["T"]).min() > 0.05


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_families_are_what_they_say(seed):
    W, H = C.W_SCENE, C.H_SCENE
    assert _is_aniso(C.family("aniso", W, H, seed))
    assert (C.family("aniso", W, H, seed)["K"][0, 0] > C.family("aniso", W, H, seed)["K"][1, 1]) == (seed % 2 == 0)
    off = C.family("offcentre", W, H, seed)
    assert _is_offcentre(off)
    assert (off["K"][0, 2] > W / 2) == bool(seed & 1) and (off["K"][1, 2] > H / 2) == bool(seed & 2)
    assert _is_rolled(C.family("rolled", W, H, seed))
    np.testing.assert_allclose(np.degrees(C.family("narrow", W, H, seed)["FoVy"]), 12.0, rtol=1e-12)
    np.testing.assert_allclose(np.degrees(C.family("wide", W, H, seed)["FoVy"]), 110.0, rtol=1e-12)
    for name in ("aniso", "offcentre", "rolled", "narrow", "wide"):       # none of these truncates by accident
        cam = C.family(name, W, H, seed)
        assert _bsize(cam) == (cam["W"], cam["H"]), name


def test_trunc_family_truncates_and_its_sibling_does_not():
    t, x = C.family("trunc", C.W_SCENE, C.H_SCENE, 0), C.family("trunc_x", C.W_SCENE, C.H_SCENE, 0)
    assert (t["W"], t["H"]) == (x["W"], x["H"])
    assert 0 <= t["W"] - C.W_SCENE < 16 and 0 <= t["H"] - C.H_SCENE < 16
    assert _bsize(t) == (t["W"] - 1, t["H"] - 1)
    assert _bsize(x) == (x["W"] - 1, x["H"])
    assert t["tanfovx"] == x["tanfovx"] and 0 < abs(t["tanfovy"] / x["tanfovy"] - 1) < 1e-4


def test_trunc_scene_shows_the_truncation_in_the_scale_gradient():
    """The float32 oracle under trunc and under its sibling (same Gaussians, fy a few ulps away): forwards equal to 2e-4, dL_dscales
    apart by about 1 / H.  tests/test_gpu_cameras.py asserts more than 1e-3 between the two HIP runs; this is the margin it has."""
    from helpers import assert_image_close, rel_maxnorm
    kw, kw_x, cam = C.trunc_pair()
    g = C.S.make_upstream_grads(cam["H"], cam["W"], C.SEEDS["trunc"])
    res = []
    for k in (kw, kw_x):
        o = orc.SurfelOracle(np.float32)
        ref = o.forward(**k)
        res.append((ref, o.backward(dL_dcolor=g["dL_dcolor"], dL_dallmap=g["dL_dplanes"], dL_drefl_strength_map=g["dL_drefl"])))
    # one ulp of the float32 projection entry moves a centre by about 1e-5 px, and the colour of an edge-on surfel changes by several units
    # per pixel: the forwards agree to 2e-4 (a pair on a blend threshold may flip: helpers.assert_image_close), 40 times closer than the gradients
    assert_image_close(res[1][0]["color"], res[0][0]["color"], 2e-4)
    diff = rel_maxnorm(res[1][1]["dL_dscales"], res[0][1]["dL_dscales"])
    print("trunc against trunc_x, dL_dscales (oracle):", diff)
    assert 3e-3 < diff < 10.0 / cam["H"]


def test_backward_size_restates_the_float32_expression():
    """The pairs found by hand on a grid of widths and FoVs of make_camera's form: (200, 20 deg), (256, 20 deg), (256, 75 deg) and
    (800, 20 deg) truncate; the nine sizes the rest of the suite renders at 50 deg do not."""
    import math
    for n, deg in ((200, 20.0), (256, 20.0), (256, 75.0), (800, 20.0)):
        assert C.backward_size(n, math.tan(math.radians(deg) * 0.5)) == n - 1, (n, deg)


@pytest.mark.parametrize("seed", [70, 71])
def test_all_family_is_everything_at_once(seed):
    cam = C.family("all", C.W_SCENE, C.H_SCENE, seed)
    assert _is_aniso(cam) and _is_offcentre(cam) and _is_rolled(cam)
    assert _bsize(cam) == (cam["W"] - 1, cam["H"] - 1)


@pytest.mark.parametrize("name", ["aniso", "offcentre", "all"])
def test_view_rays_differ_from_those_of_a_centred_square_pixel_camera(name):
    """The float64 reference chain's unit view rays under the family's K against the rays of the K a kernel would see if it read K[0][0]
    alone (fy = fx, principal point at the centre): nearly every pixel differs by far more than the reflection's forward bar
    (helpers_refl.fwd_bar), so tests/test_gpu_camera_passes.py cannot pass with such a kernel."""
    import helpers_refl as R
    cam = C.family(name, R.SEAM_W, R.SEAM_H, 11)
    centred = dict(cam, K=np.array([[cam["K"][0, 0], 0, cam["W"] / 2], [0, cam["K"][0, 0], cam["H"] / 2], [0, 0, 1]], np.float32))
    d = np.abs(R.view_rays(cam, cam["W"], cam["H"]) - R.view_rays(centred, cam["W"], cam["H"])).max(axis=1)
    assert (d > 100 * R.fwd_bar(16)).mean() > 0.9, (d.min(), d.max())


# ------------------------------------------------------------------------------------------- reach of the scenes, float32 oracle
@pytest.mark.parametrize("variant", ["S", "G"])
@pytest.mark.parametrize("name", C.FAMILIES + ("trunc_x",))
def test_scene_reach(name, variant):
    kw, cam = C.scene(name, variant)
    P = kw["means3D"].shape[0]
    o = (orc.SurfelOracle if variant == "S" else orc.GaussOracle)(np.float32)
    o.forward(**kw)
    vis = o.state("radii") > 0
    V = kw["viewmatrix"].astype(np.float64)
    t = kw["means3D"].astype(np.float64) @ V[:3, :3] + V[3, :3]
    px = cam["K"][0, 0] * t[:, 0] / t[:, 2] + cam["K"][0, 2] - 0.5
    py = cam["K"][1, 1] * t[:, 1] / t[:, 2] + cam["K"][1, 2] - 0.5
    offscreen = (px < 0) | (px > cam["W"] - 1) | (py < 0) | (py > cam["H"] - 1)
    counts = dict(visible=int(vis.sum()), near_culled=int((t[:, 2] <= 0.2).sum()), offscreen=int(offscreen.sum()),
                  offscreen_visible=int((offscreen & vis).sum()))
    assert counts["visible"] >= 0.3 * P, counts
    assert counts["near_culled"] >= 0.03 * P, counts
    assert counts["offscreen"] >= 0.3 * P and counts["offscreen_visible"] >= 100, counts
    if variant == "G":
        cx, cy = C.clamp_classes(kw)
        counts.update(clamped_x=int((vis & cx).sum()), clamped_y=int((vis & cy).sum()), clamped_xy=int((vis & cx & cy).sum()))
        assert counts["clamped_x"] >= 50 and counts["clamped_y"] >= 50 and counts["clamped_xy"] >= 10, counts
    print(name, variant, cam["W"], cam["H"], counts)
