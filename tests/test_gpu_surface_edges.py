"""Surface pass (csrc/gsr_surface.hip) against the float64 oracle per element, within the error bounds of
tests/loss_bounds.py: every 16-pixel tile offset with its halo of 1 (forward) and 2 (backward), depth_ratio 0 / 0.3 / 1,
alpha at the clamp, non-finite depths, cross products below the normalize eps or exactly zero, and each set of cotangents
(both, surf_depth only, surf_normal only: the NULL paths of gsr_surface_backward).  Complements the 1e-3-of-max checks of
test_gpu_surface.py."""
import numpy as np
import pytest
import torch

import loss_bounds as LB

pytestmark = pytest.mark.gpu
RATIOS = (0.0, 0.3, 1.0)
MODES = ("both", "depth_only", "normal_only")


def gpu_surface(am, ray, ratio, gsd, gsn):
    """C ABI forward and backward; outputs pre-filled with NaN so that an element the kernels never write fails."""
    from _gsr import check, lib, stream_ptr
    A, R = torch.from_numpy(am).cuda(), torch.from_numpy(ray).cuda()
    H, W = am.shape[1], am.shape[2]
    sd = torch.full((H, W), float("nan"), device="cuda")
    sn = torch.full((3, H, W), float("nan"), device="cuda")
    s = stream_ptr(A.device)
    check(lib.gsr_surface_forward(A.data_ptr(), R.data_ptr(), float(ratio), H, W, sd.data_ptr(), sn.data_ptr(), s), "gsr_surface_forward")
    GD = None if gsd is None else torch.from_numpy(gsd).cuda()
    GN = None if gsn is None else torch.from_numpy(gsn).cuda()
    g = torch.full((8, H, W), float("nan"), device="cuda")
    check(lib.gsr_surface_backward(A.data_ptr(), R.data_ptr(), float(ratio), H, W, sd.data_ptr(), None if GD is None else GD.data_ptr(),
                                   None if GN is None else GN.data_ptr(), g.data_ptr(), s), "gsr_surface_backward")
    torch.cuda.synchronize()
    return sd.cpu().numpy(), sn.cpu().numpy(), g.cpu().numpy()


def cotangents(H, W, mode, seed):
    rs = np.random.RandomState(seed)
    gsd = rs.randn(H, W).astype(np.float32) if mode != "normal_only" else None
    gsn = rs.randn(3, H, W).astype(np.float32) if mode != "depth_only" else None
    return gsd, gsn


def check_surface(am, ray, ratio, mode, seed, what):
    H, W = am.shape[1], am.shape[2]
    gsd, gsn = cotangents(H, W, mode, seed)
    ref, bnd, skip = LB.surface_reference(am, ray, ratio, gsd, gsn)
    sd, sn, g = gpu_surface(am, ray, ratio, gsd, gsn)
    LB.check(sd, ref["sd"], bnd["sd"], skip["sd"], f"{what} surf_depth")
    LB.check(sn, ref["sn"], bnd["sn"], skip["sn"], f"{what} surf_normal")
    LB.check(g, ref["g"], bnd["g"], skip["g"], f"{what} g_allmap")
    assert (g[[2, 3, 4, 6, 7]] == 0).all(), what
    return ref, (sd, sn, g)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ratio", RATIOS)
def test_tile_offsets_and_branches(ratio, mode):
    """All H, W in SURF_SIZES; the smooth scene and the branch scene alternate."""
    k = 0
    for H in LB.SURF_SIZES:
        for W in LB.SURF_SIZES:
            k += 1
            if k % 2:
                am, ray = LB.surface_scene(H, W, k)
            else:
                am, ray = LB.surface_branch_scene(H, W, k, ratio)
            check_surface(am, ray, ratio, mode, 1000 + k, f"{H}x{W} ratio={ratio} {mode}")


@pytest.mark.parametrize("ratio", RATIOS)
def test_branch_values_are_reached(ratio):
    """The branch scene reaches what it is meant to: alpha at and one ulp around the clamp with a non-zero alpha gradient
    exactly from fl32(1e-3) up, cross products below 1e-12 with a non-zero gradient, NaN classes where the depth is not
    finite, and the kernel agrees with the reference at each."""
    H, W = 34, 33
    am, ray = LB.surface_branch_scene(H, W, 5, ratio)
    ref, (sd, sn, g) = check_surface(am, ray, ratio, "both", 5, f"branch ratio={ratio}")
    A = am[1]
    at, below = A == np.float32(LB.ALPHA_MIN), A == np.float32(LB.ALPHA_CASES[1])
    assert at.sum() >= 4 and below.sum() >= 4
    if ratio < 1.0:
        fin = np.isfinite(am[0])
        assert (np.abs(ref["g"][1][at & fin]) > 0).any() and (np.abs(g[1][at & fin]) > 0).any()
    assert (g[1][below] == 0).all() and (g[1][A == 0] == 0).all()
    # |c| < 1e-12 in the tiny-depth rows (interior pixels with non-zero alpha): the gradient there is large and matched
    rows = np.arange(H)[:, None] % 9
    tiny = np.broadcast_to((rows == 5), (H, W)).copy()
    tiny[:, [0, W - 1]] = False
    assert (np.abs(g[0][tiny]) > 0).any() or ratio == 1.0
    assert np.isnan(ref["g"][1]).any() == np.isnan(g[1]).any()


@pytest.mark.parametrize("mode", MODES)
def test_full_size_synthetic(mode):
    am, ray = LB.surface_scene(1080, 1920, 41, LB.pinhole_raymat(1080, 1920, f=1400.0))
    check_surface(am, ray, 0.3, mode, 41, f"1080p synthetic {mode}")


def test_full_size_rasterized_allmap():
    """The allmap the rasterizer produces for a synthetic scene at 1080p, with the camera's own ray block."""
    import gsr_synth as S
    from diff_surfel_rasterization import GaussianRasterizer
    from gaussian_renderer import _ray_block, _settings
    P, W, H = 1_000_000, 1920, 1080           # the C3 configuration's size
    sc = S.make_scene(P, "S", seed=37)
    cam = S.make_camera(W, H)
    ct = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cam.items() if isinstance(v, np.ndarray)}

    class View:
        FoVx, FoVy = 2 * np.arctan(cam["tanfovx"]), 2 * np.arctan(cam["tanfovy"])
        image_width, image_height = W, H
        world_view_transform, full_proj_transform, camera_center = ct["viewmatrix"], ct["projmatrix"], ct["campos"]
        znear, zfar = 0.01, 100.0

    class PC:
        get_xyz, get_opacity, get_scaling, get_rotation, get_features, get_refl = (
            torch.from_numpy(sc["means3D"]).cuda(), torch.from_numpy(sc["opacities"]).cuda(), torch.from_numpy(sc["scales"]).cuda(),
            torch.from_numpy(sc["rotations"]).cuda(), torch.from_numpy(sc["shs"]).cuda(), torch.from_numpy(sc["refl_strengths"]).cuda())
        active_sh_degree = 3
    with torch.no_grad():
        rast = GaussianRasterizer(raster_settings=_settings(View, PC, torch.zeros(3, device="cuda"), 1.0))
        _, _, allmap, _, _ = rast(means3D=PC.get_xyz, means2D=torch.zeros(P, 3, device="cuda"), shs=PC.get_features,
                                  refl_strengths=PC.get_refl, opacities=PC.get_opacity, scales=PC.get_scaling, rotations=PC.get_rotation,
                                  env_scope_mask=torch.ones(P, dtype=torch.bool, device="cuda"))
        ray = _ray_block(View)
    am = np.ascontiguousarray(allmap.float().cpu().numpy())
    assert (am[1] > 0.5).mean() > 0.05              # the scene covers a good part of the image
    check_surface(am, ray.float().cpu().numpy(), 0.3, "both", 43, "1080p rasterized")
