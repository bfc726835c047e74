"""GPU: the pixel passes that read a camera — the surface pass with its ray block, the deferred reflection with its camera block
(shading normal, view rays through K^-1, every backward path), the fused rasterize + reflect node and render() itself — under the
camera families of tests/cameras.py, whose views (cameras.view_of) carry the family's own K in HWK.  Each is held to the float64
reference and the bars of the existing test of the same pass, imported from it:
  surface pass        tests/test_gpu_surface_edges.py check_surface (loss_bounds.surface_reference), on an allmap rasterized under the camera
  deferred reflection tests/helpers_refl.py check_path (reference chain, ambiguity classifier and envelope), as test_gpu_refl_seams.py
  fused node          tests/test_gpu_fused.py: the rasterizer's outputs bit for bit, reflection outputs 5e-6, gradients 5e-5
  render()            tests/test_gpu_render_options.py _run_case, stages A - D (with compute_cov3D_python: render_ref.python_path_gradients)
With square pixels and a centred principal point, K[0][0] for K[1][1], W/2 for H/2 or cx for W/2 can be swapped in any of them unseen."""
import numpy as np
import pytest
import torch

import cameras as C
import helpers_refl as R
from helpers import HipSurfel, S, rel_maxnorm

pytestmark = pytest.mark.gpu
W, H = 160, 96
SEEDS = {"aniso": 11, "offcentre": 21, "rolled": 31, "all": 71}


# ------------------------------------------------------------------------------------------- surface pass
def ray_block_ref(cam):
    """float64 [12] of gaussian_renderer._ray_block: rays_d(x, y) = (x, y, 1) @ M, M = intrins^-1.T @ c2w[:3, :3].T, then the camera
    centre.  The reference derives `intrins` from full_proj_transform with an NDC-to-pixel matrix centred at (W/2, H/2)
    (utils/point_utils.py): pixel x = (ndc.x + 1) W / 2 = fx x / z + cx with the projection of cameras.hwk_camera, so intrins is K
    itself — the principal point as given, not moved by the half pixel the rasterizers' ndc2pix takes off."""
    K = np.asarray(cam["K"], np.float64)
    M = np.linalg.inv(K).T @ np.asarray(cam["R"], np.float64).T
    return np.concatenate([M.reshape(-1), np.asarray(cam["campos"], np.float64)])


@pytest.mark.parametrize("name", ["aniso", "offcentre", "rolled", "all"])
def test_surface_pass_under_camera_family(name):
    from gaussian_renderer import _ray_block
    from test_gpu_surface_edges import check_surface
    cam = C.family(name, W, H, SEEDS[name])
    kw = C.frustum_scene("S", 2000, cam, 200 + SEEDS[name])
    am = HipSurfel(kw, requires_grad=False).out()["allmap"]
    assert am.shape == (8, cam["H"], cam["W"]) and (am[1] > 0.5).mean() > 0.05
    ray = _ray_block(C.view_of(cam)).float().cpu().numpy()
    want = ray_block_ref(cam)
    err = np.abs(ray[:9].reshape(3, 3) - want[:9].reshape(3, 3)) / np.abs(want[:9].reshape(3, 3)).max(axis=1, keepdims=True)
    print(f"{name}: ray block off by {err.max():.2e} of its row, centre by {np.abs(ray[9:] - want[9:]).max():.2e}")
    # two float32 inversions of 3 x 3 matrices whose condition number is about the focal length in pixels (up to 270 here), 2^-24 each:
    # 1e-5 bounds them; a swapped focal length moves M by 0.3 of its row, a centred principal point by 0.1
    assert err.max() <= 1e-5 and np.abs(ray[9:] - want[9:]).max() <= 1e-5
    for ratio, mode in ((0.3, "both"), (1.0, "normal_only"), (0.0, "depth_only")):
        check_surface(np.ascontiguousarray(am), ray, ratio, mode, 300 + SEEDS[name], f"{name} ratio={ratio} {mode}")


# ------------------------------------------------------------------------------------------- deferred reflection, two-node
@pytest.mark.parametrize("name", ["aniso", "offcentre", "rolled"])
def test_deferred_reflection_under_camera_family(name):
    """test_gpu_refl_seams.test_deferred_reflection_at_seams at L = 16 under the family's camera: forward planes (shading_normal is the
    nworld plane), per-pixel and texel gradients on every path (both REFLECTION_BACKWARD_BINNED settings among them)."""
    cam = C.family(name, R.SEAM_W, R.SEAM_H, SEEDS[name])
    inp = R.seam_inputs(16, seed=SEEDS[name], cam=cam)
    ref = R.reference_run(inp)
    env = R.envelope(inp, ref)
    fails = []
    for path in R.PATHS:
        obs, f = R.check_path(inp, ref, env, (R.hip_run(inp, path, False), R.hip_run(inp, path, True)), path)
        print(name, path, {k: round(v, 4) for k, v in obs.items()})
        fails += f
    assert not fails, fails


@pytest.mark.parametrize("name", ["aniso", "offcentre", "rolled"])
def test_shading_normal_under_camera_family(name):
    from gaussian_renderer import shading_normal
    from helpers_chain import reference_dirs
    cam = C.family(name, W, H, SEEDS[name])
    v = C.view_of(cam)
    g = torch.Generator().manual_seed(SEEDS[name])
    nv = (torch.randn(3, H, W, generator=g) * torch.rand(1, H, W, generator=g)).cuda().requires_grad_(True)
    w = torch.randn(3, H, W, generator=g)
    out = shading_normal(nv, v.world_view_transform, v.HWK, v.R, v.T)
    (out * w.cuda()).sum().backward()
    nv64 = nv.detach().cpu().double().requires_grad_(True)
    rn, _, _ = reference_dirs(nv64, cam, W, H)
    (rn.permute(2, 0, 1) * w.double()).sum().backward()
    assert float((out.detach().cpu().double() - rn.detach().permute(2, 0, 1)).abs().max()) <= R.fwd_bar(16)
    assert rel_maxnorm(nv.grad.cpu().numpy(), nv64.grad.numpy()) <= 1e-4


# ------------------------------------------------------------------------------------------- fused node and render()
@pytest.mark.parametrize("name", ["aniso", "offcentre", "rolled", "all"])
def test_fused_node_equals_two_nodes_under_camera_family(name):
    """tests/test_gpu_fused.py::test_fused_equals_rasterizer_then_reflection on the family's scene: the fused rasterize_reflect node
    against GaussianRasterizer followed by deferred_reflection(), which the tests above hold to float64 under the same cameras."""
    from test_gpu_fused import PARAMS, _run, _upstream
    cam = C.family(name, W, H, SEEDS[name])
    w, h = cam["W"], cam["H"]
    kw = C.frustum_scene("S", 3000, cam, 400 + SEEDS[name])
    tex, fail = S.make_cubemap(16, 3, 400)
    src = {k: torch.from_numpy(kw[k]).cuda() for k in ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")}
    src["cubemap"], src["fail"] = torch.from_numpy(tex).cuda(), torch.from_numpy(fail).cuda() + 0.25
    mask = torch.from_numpy(kw["env_scope_mask"]).cuda()
    ct, bg = C.view_of(cam).ct, torch.tensor((0.1, 0.2, 0.3), device="cuda")
    ups = _upstream(h, w, 4)
    res = {}
    for fused in (False, True):
        p = {k: v.clone().requires_grad_(True) for k, v in src.items()}
        out, g2d = _run(fused, p, mask, cam, ct, w, h, bg, ups)
        res[fused] = (out, {k: p[k].grad for k in PARAMS}, g2d)
    (ou, gu, mu_), (of, gf, mf) = res[False], res[True]
    for k in ("base", "radii", "allmap", "refl_map", "gw"):
        assert torch.equal(ou[k], of[k]), k
    for k in ("final", "refl_color", "nworld"):
        assert float((ou[k] - of[k]).abs().max()) <= 5e-6, k
    assert float(of["final"].abs().max()) > 0.1 and float(of["allmap"][1].max()) > 0.5
    for k in PARAMS:
        a, b = gf[k].cpu().numpy(), gu[k].cpu().numpy()
        assert np.isfinite(a).all() and (k == "fail" or np.abs(b).max() > 0), k
        print(name, "fused against two nodes", k, rel_maxnorm(a, b))
        assert rel_maxnorm(a, b) <= 5e-5, k
    assert rel_maxnorm(mf.cpu().numpy(), mu_.cpu().numpy()) <= 5e-5


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two-nodes"])
@pytest.mark.parametrize("pycov", [False, True], ids=["hip-T", "pycov"])
def test_render_under_all(pycov, fused, monkeypatch):
    """tests/test_gpu_render_options.py::test_render_option ("default" and "pycov") with its camera and scene replaced by `all` and a
    frustum scene under it: rasterizer against the oracle, pixel passes against float64, gradients through to the parameters, and with
    compute_cov3D_python the Python homographies and render_ref.python_path_gradients, at that test's bars and floors."""
    import test_gpu_render_options as RO
    cam = C.family("all", RO.W, RO.H, 70)
    assert (cam["W"], cam["H"]) == (RO.W, RO.H)         # (the truncation search found this size itself)
    kw = C.frustum_scene("S", RO.P, cam, 500)
    rs = np.random.RandomState(500)
    sc = {k: kw[k] for k in RO.NAMES}
    sc["rotations"] = (sc["rotations"] * rs.uniform(0.5, 2.0, (RO.P, 1))).astype(np.float32)       # raw quaternions, as RO._data
    tex, fail = S.make_cubemap(RO.L, 3, 500)
    data = (sc, tex, fail + np.float32(0.25), rs.rand(RO.P, 3).astype(np.float32))
    monkeypatch.setattr(RO, "_camera", lambda: cam)
    monkeypatch.setattr(RO, "_data", lambda: data)
    RO._run_case(monkeypatch, fused, compute_cov3D_python=pycov)
